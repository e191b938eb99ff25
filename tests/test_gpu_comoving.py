"""The comoving radiation field on the device (mcrat_hip_comoving_field, mcrat_hip_pool_comoving_field; mcrat_amd/csrc/comoving.hip) against
tests/comoving_checker.py, an independent NumPy restatement of the definitions (include/mcrat_hip.h) that finds the cell by
brute force, takes the cell's velocity from synth.hydro_vector_to_cartesian and both the fluid-frame energy and the fluid-frame cosine from a
textbook boost -- not from the closed form the kernel evaluates.

Exact: n_observable, n_unlocated, n_outside and the count per bin -- no committed case holds a photon within 1e-9 of a cell's size of a face, or
within twice its conditioning bar of an energy or cosine edge (tests/test_comoving_checker_cpu.py), so the window a fragile photon would be granted
is of width zero.  Sums, per bin with n terms t_i of the checker, u = 2^-53 (the derivation: tests/comoving_checker.py):
    w, we_lab, wem, wemm   |dev - chk| <= (n + 2) u sum|t_i|                     (the terms are the same bits on both sides; any summation order)
    we                     ... + sum 2 bar_e |t_i|,   bar_e = 8u (1 + |x|)(1 + Gamma^2) / (1 - x),  x = v.p / p0
    wea                    ... + sum (2 bar_e |a| + d) |w e|,   d = 2 bar_a,  bar_a = 8u (3 + |a| b) / (1 - x)
    weaa                   ... + sum (2 bar_e a^2 + 2 |a| d + d^2) |w e|
Derived, not measured; a bin nobody is in has the bound 0: its planes must hold exactly 0.  The largest error / bound is printed per case.
Oracle-free on the device's own planes: the counter identity, |wea| <= we and 0 <= weaa <= we (the lab planes likewise), the planes summed over e
and a against mcrat_hip_radiation_field, and isotropic radiation's H / J = 0 and K / J = 1 / 3."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import comoving_checker as cc
from tests import radfield_checker as rc
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

CYL = (synth.TWO, synth.CYLINDRICAL)
EVERY_E = np.array([0.0, 1e300])                        # edges that cover every energy and every cosine
EVERY_A = np.array([-1.0, 2.0])


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(autouse=True)
def no_forced_path(monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_COMOVING_PATH", raising=False)
    monkeypatch.delenv("MCRAT_HIP_RADFIELD_PATH", raising=False)


def engine_for(hip, frame, ph=None):
    e = hip.Engine(frame["dimensions"], frame["geometry"], 0)
    e.set_hydro(frame)
    if ph is not None:
        e.set_photons(ph)
    return e


def invariants(res, label, slack=None):
    """what holds for the device's planes whatever the checker says; slack: dict of per-bin bounds for the inequalities between sums"""
    assert int(res["count"].sum()) + res["n_unlocated"] + res["n_outside"] == res["n_observable"], label
    zero = lambda k: slack[k] if slack is not None else 0.0
    for e, first, second in (("we", "wea", "weaa"), ("we_lab", "wem", "wemm")):
        assert (res[e] >= 0).all() and (res["w"] >= 0).all(), (label, e)
        assert (np.abs(res[first]) <= res[e] + zero("bound_" + first) + zero("bound_" + e)).all(), (label, first)
        assert (res[second] >= -zero("bound_" + second)).all() and (res[second] <= res[e] + zero("bound_" + second) + zero("bound_" + e)).all(), (label, second)
    for k in cc.SUMS:
        assert not res[k][res["count"] == 0].any(), (label, k)


def compare(res, want, label, fragile_ok=False):
    assert fragile_ok or want["n_fragile"] == 0, label
    assert res["count"].shape == want["count"].shape and res["count"].dtype == np.int64, label
    for k in ("n_observable", "n_unlocated"):
        assert res[k] == want[k], (label, k, res[k], want[k])
    # per bin: the checker's count with the fragile photons removed ... and with them added (no committed case holds one: equality)
    lo, hi = want["count_sure"], want["count_sure"] + want["n_fragile"]
    assert ((res["count"] >= lo) & (res["count"] <= hi)).all(), (label, np.argwhere((res["count"] < lo) | (res["count"] > hi))[:8])
    assert abs(res["n_outside"] - want["n_outside"]) <= want["n_fragile"], (label, res["n_outside"], want["n_outside"])
    if want["n_fragile"] == 0:
        assert np.array_equal(res["count"], want["count"]) and res["n_outside"] == want["n_outside"], label
    invariants(res, label, want)
    worst = {}
    for k in cc.SUMS:
        err, bound = np.abs(res[k] - want[k]), want["bound_" + k]
        worst[k] = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    print("%s: %d counted, %d bins in use; largest error / bound: %s" % (label, int(want["count"].sum()), int((want["count"] > 0).sum()),
                                                                         ", ".join("%s %.3g" % (k, worst[k]) for k in cc.SUMS)))
    if want["n_fragile"] == 0:
        for k in cc.SUMS:
            assert (np.abs(res[k] - want[k]) <= want["bound_" + k]).all(), (label, k, worst[k])      # (an empty bin: bound 0, the device's plane must hold 0)


def shells_args(mode):
    return (cc.SHELL_R, cc.SHELL_MU) if mode == cc.SHELLS else ()


def run_case(hip, name, mode, **kw):
    c = cc.case(name)
    e = engine_for(hip, c["frame"], c["ph"])
    res = e.comoving_field(mode, cc.E_EDGES, cc.A_EDGES, *shells_args(mode), **kw)
    path = e.comoving_field_path()
    e.close()
    return c, res, path


# ---------------------------------------------------------------------------------------------- sizes, geometries, Lorentz factors
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1000])
def test_ragged_sizes_in_both_modes(hip, n):
    name = "cells_n%d" % n
    c, res, path = run_case(hip, name, cc.CELLS)
    assert res["w"].shape == (256, 6, 4) and path == hip.COMOVING_PATH_GLOBAL
    compare(res, cc.want(name, cc.CELLS), "CELLS, n = %d" % n)
    c, res, path = run_case(hip, name, cc.SHELLS)
    assert res["w"].shape == (8, 4, 6, 4) and path == hip.COMOVING_PATH_LDS
    compare(res, cc.want(name, cc.SHELLS), "SHELLS, n = %d" % n)


@pytest.mark.parametrize("dims, geom", sc.PAIRS)
def test_every_dimensions_geometry_pair(hip, dims, geom):
    name = "pair_%d_%d" % (dims, geom)
    c, res, path = run_case(hip, name, cc.CELLS)
    assert path == hip.COMOVING_PATH_GLOBAL and res["count"].shape == (c["frame"]["num_elements"], 6, 4)
    compare(res, cc.want(name, cc.CELLS), "CELLS, DIMENSIONS %d, geometry %d" % (dims, geom))
    assert res["count"].sum() > 100 and (res["count"] > 0).sum() > 50
    c, res, path = run_case(hip, name, cc.SHELLS)
    assert path == hip.COMOVING_PATH_LDS and res["count"].shape == (8, 4, 6, 4)
    compare(res, cc.want(name, cc.SHELLS), "SHELLS 8 x 4, DIMENSIONS %d, geometry %d" % (dims, geom))
    assert res["count"].sum() > 20


def test_lorentz_factors_up_to_100(hip):
    for mode in (cc.CELLS, cc.SHELLS):
        c, res, _ = run_case(hip, "gamma_100", mode)
        compare(res, cc.want("gamma_100", mode), "gamma_max 100, mode %d" % mode)
    assert c["frame"]["gamma"].max() > 80
    # the boost matters: the fluid-frame moments are far from the lab's about the flow
    w = cc.want("gamma_100", cc.CELLS)
    used = w["count"] > 0
    assert (np.abs(w["we"] - w["we_lab"]) > 1e6 * w["bound_we"])[used].all()


@pytest.mark.parametrize("name", ["crowded_4", "crowded_1", "spread"])
def test_crowded_and_spread(hip, name):
    """1000 photons in four cells and in one (same-address adds, the in-wave grouping), and in 1000 different cells of a 32 x 32 mesh (nearly every
    lane alone): the global path's rounds"""
    c, res, path = run_case(hip, name, cc.CELLS)
    assert path == hip.COMOVING_PATH_GLOBAL
    want = cc.want(name, cc.CELLS)
    compare(res, want, name)
    in_use = int((res["count"].sum(axis=(1, 2)) > 0).sum())
    assert res["count"].sum() + res["n_outside"] == 1000 and res["count"].sum() > 900
    assert in_use == {"crowded_4": 4, "crowded_1": 1}[name] if name != "spread" else in_use > 900
    assert res["count"].max() >= {"crowded_4": 10, "crowded_1": 38, "spread": 1}[name]      # (more than 900 photons in 4 x 24 and in 24 bins)
    if name == "spread":                                   # one term per bin: the equal-bits sums are the terms themselves
        ph, b = c["ph"], want["bin"]
        at = b >= 0
        wl = ph["weight"] * (ph["p0"] * synth.C_LIGHT)
        for k, t in (("w", ph["weight"]), ("we_lab", wl), ("wem", wl * want["q"]["m"]), ("wemm", (wl * want["q"]["m"]) * want["q"]["m"])):
            assert np.array_equal(res[k].ravel()[b[at]], t[at]), k


def test_gap_domain_and_slots_that_do_not_count(hip):
    """a slab with a gap and photons beyond the domain: n_unlocated; weight 0, 'p', 'N': not counted; 'c' counted"""
    c, res, _ = run_case(hip, "gap", cc.CELLS)
    want = cc.want("gap", cc.CELLS)
    compare(res, want, "gap")
    ph = c["ph"]
    n = len(ph["weight"])
    observable = (ph["weight"] != 0) & (ph["type"] != b"p") & (ph["type"] != b"N")
    assert res["n_observable"] == observable.sum() < n - 200 and ((ph["type"] == b"c") & (want["bin"] >= 0)).sum() > 30
    for excluded in (ph["weight"] == 0, ph["type"] == b"p", ph["type"] == b"N"):
        assert excluded.sum() > 50 and (want["bin"][excluded] < 0).all()
    whole = cc.field(c["whole"], ph, cc.CELLS, cc.E_EDGES, cc.A_EDGES)
    assert res["n_unlocated"] > whole["n_unlocated"] + 20 > 30
    c, res, _ = run_case(hip, "gap", cc.SHELLS)
    compare(res, cc.want("gap", cc.SHELLS), "gap, SHELLS")
    assert res["n_unlocated"] == want["n_unlocated"] and res["n_outside"] > want["n_outside"]


def test_cells_at_rest_take_the_radial_cosine(hip):
    """every third cell of the frame has v = 0: there a is m and e is e_lab, the same bits -- the fluid-frame planes of those cells equal the lab
    planes where each holds one photon, and agree within the summation bound where it holds more"""
    for mode in (cc.CELLS, cc.SHELLS):
        c, res, _ = run_case(hip, "rest", mode)
        compare(res, cc.want("rest", mode), "cells at rest, mode %d" % mode)
    c, res, _ = run_case(hip, "rest", cc.CELLS)
    want = cc.want("rest", cc.CELLS)
    still = np.nonzero(c["frame"]["gamma"] == 1.0)[0]
    assert len(still) == 86 and res["count"][still].sum() > 150
    one = res["count"][still] == 1
    assert one.sum() > 20
    for k, kl in (("we", "we_lab"), ("wea", "wem"), ("weaa", "wemm")):
        assert np.array_equal(res[k][still][one].view(np.int64), res[kl][still][one].view(np.int64)), k
        assert (np.abs(res[k][still] - res[kl][still]) <= 2 * want["bound_" + kl][still]).all(), k
    moving = np.setdiff1d(np.arange(256), still)
    assert (res["we"][moving] != res["we_lab"][moving])[res["count"][moving] > 0].all()


# ---------------------------------------------------------------------------------------------- paths
def test_lds_and_global_paths_agree(hip, monkeypatch):
    c = cc.case("shells")
    want = cc.want("shells", cc.SHELLS)
    e = engine_for(hip, c["frame"], c["ph"])
    assert e.comoving_field_path() == 0
    got = {}
    for path, code in (("lds", hip.COMOVING_PATH_LDS), ("global", hip.COMOVING_PATH_GLOBAL)):
        monkeypatch.setenv("MCRAT_HIP_COMOVING_PATH", path)
        got[path] = e.comoving_field(cc.SHELLS, cc.E_EDGES, cc.A_EDGES, cc.SHELL_R, cc.SHELL_MU)
        assert e.comoving_field_path() == code
        compare(got[path], want, "SHELLS 8 x 4 x 6 x 4, 1000 photons, " + path)
    assert np.array_equal(got["lds"]["count"], got["global"]["count"])
    for k in cc.SUMS:
        assert (np.abs(got["lds"][k] - got["global"][k]) <= 2 * want["bound_" + k]).all(), k
    assert want["n_outside"] > 20 and (want["count"] > 0).sum() > 100
    monkeypatch.setenv("MCRAT_HIP_COMOVING_PATH", "lds")
    with pytest.raises(hip.McratHipError, match="CELLS always accumulates in global memory"):
        e.comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES)
    monkeypatch.setenv("MCRAT_HIP_COMOVING_PATH", "global")
    compare(e.comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES), cc.want("shells", cc.CELLS), "CELLS, global asked for")
    e.close()


@pytest.mark.parametrize("n_e, lds", [(1136, True), (1137, False)])
def test_path_changes_at_the_lds_budget(hip, n_e, lds):
    """1 x 1 x 1136 x 1 bins with their edges and counters are 81 872 B of LDS, the last shape that fits 80 KiB; one energy more and the planes stay
    in HBM (tests/test_comoving_plan_cpu.py has the rule)"""
    c = cc.case("shells")
    e_edges = 10.0 ** np.linspace(-11.513, -4.487, n_e + 1)
    r_edges, mu_edges, a_edges = np.array([1.0e12, 1.2e12]), np.array([0.9, np.nextafter(1.0, 2.0)]), np.array([-1.0, np.nextafter(1.0, 2.0)])
    want = cc.field(c["frame"], c["ph"], cc.SHELLS, e_edges, a_edges, r_edges, mu_edges)
    e = engine_for(hip, c["frame"], c["ph"])
    res = e.comoving_field(cc.SHELLS, e_edges, a_edges, r_edges, mu_edges)
    assert e.comoving_field_path() == (hip.COMOVING_PATH_LDS if lds else hip.COMOVING_PATH_GLOBAL)
    e.close()
    assert res["count"].shape == (1, 1, n_e, 1)
    compare(res, want, "1 x 1 x %d x 1" % n_e)
    assert (want["count"] > 0).sum() > 300 and want["count"][0, 0, -300:].sum() > 0 and want["count"][0, 0, :300].sum() > 0


# ---------------------------------------------------------------------------------------------- half-open edges
def uniform_frame(v0, v1, gamma, open_axis=True):
    frame = sc.mesh(*CYL)
    m = frame["num_elements"]
    frame.update(v0=np.full(m, v0), v1=np.full(m, v1), gamma=np.full(m, gamma), dens_lab=np.full(m, 1e-10), temp=np.full(m, 3e6))
    frame["dens"] = frame["dens_lab"] / gamma
    frame["pres"] = synth.A_RAD * frame["temp"] ** 4.0 / 3
    if open_axis:
        frame["r0_domain"] = (-1.0, frame["r0_domain"][1])
    return frame


def test_an_energy_on_an_inner_edge_lands_in_the_upper_bin(hip):
    """the edge is the device's own e of the photon, read from we / w of a one-photon call with weight 1 (we is then e itself, bit for bit): the test
    does not depend on how e rounds"""
    frame = sc.random_fluid(sc.mesh(*CYL), 720)
    r = rc.points_in_cells(frame, [37, 101, 190], 721)
    ph = rc.photon_list(r, rc.momenta(722, 3), 723, exclusions=False)
    ph["weight"][:] = 1.0
    one = {k: v[:1].copy() for k, v in ph.items()}
    e1 = engine_for(hip, frame, one)
    first = e1.comoving_field(cc.CELLS, EVERY_E, EVERY_A)
    e1.close()
    assert first["count"].sum() == 1 and first["w"].sum() == 1.0
    e_dev = float(first["we"].sum())
    chk = cc.field(frame, one, cc.CELLS, EVERY_E, EVERY_A)
    assert abs(e_dev - chk["q"]["e"][0]) <= 2 * chk["q"]["bar_e"][0] * e_dev and e_dev > 0
    e = engine_for(hip, frame, ph)
    for edges, where in (([0.0, e_dev, 1e300], 1), ([0.0, np.nextafter(e_dev, 1.0), 1e300], 0), ([0.0, 1e-300, e_dev], -1), ([e_dev, 1e300], 0)):
        res = e.comoving_field(cc.CELLS, edges, EVERY_A)
        invariants(res, "an energy on an edge")
        got = res["count"][37].sum(axis=1)                      # the first photon's cell, per energy bin
        if where < 0:
            assert got.sum() == 0 and res["n_outside"] >= 1     # the last edge is open: outside
        else:
            assert got[where] == 1 and got.sum() == 1, (edges, got)
    e.close()


def test_a_photon_along_the_flow_is_counted_only_when_the_top_edge_lies_above_one(hip):
    """a flow of beta = 1/2 along +z and photons along +z: bp = p0 / 2, b = 1/2, N = D = p0 / 2 without a rounding, so a == 1 exactly; photons along
    -z have a == -1 exactly.  cosine_edges closes the axis at the forward pole; a top edge of exactly 1 leaves it outside."""
    beta = 0.5
    frame = uniform_frame(0.0, beta, 1.0 / np.sqrt(1.0 - beta * beta))
    n = 40
    r = rc.points_in_cells(frame, np.arange(n) * 5, 731)
    r[0, :5], r[1, :5] = 0.0, 0.0                               # some on the polar axis
    p0 = 10.0 ** np.random.default_rng(732).uniform(-20.0, -16.0, n)
    sign = np.where(np.arange(n) % 4 == 3, -1.0, 1.0)
    ph = rc.photon_list(r, np.stack([p0, np.zeros(n), np.zeros(n), sign * p0]), 733, exclusions=False)
    a_edges = hip.cosine_edges(8)
    assert a_edges[-1] == np.nextafter(1.0, 2.0) and a_edges[0] == -1.0 and np.allclose(np.diff(a_edges), 0.25) and len(a_edges) == 9
    e = engine_for(hip, frame, ph)
    res = e.comoving_field(cc.SHELLS, EVERY_E, a_edges, [1.0e12, 1.2e12], [0.9, 1.01])
    want = cc.field(frame, ph, cc.SHELLS, EVERY_E, a_edges, [1.0e12, 1.2e12], [0.9, 1.01])
    compare(res, want, "along the flow", fragile_ok=True)          # (the checker's a is 1 within its bar: fragile at the closed pole by its own rule)
    assert res["count"][0, 0, 0].tolist() == [10, 0, 0, 0, 0, 0, 0, 30] and res["n_outside"] == 0
    # the planes say so too: wea == we and weaa == we in the forward bin, wea == -we in the backward bin, the same bits up to the summation order
    assert abs(res["wea"][0, 0, 0, 7] - res["we"][0, 0, 0, 7]) <= 64 * cc.U * res["we"][0, 0, 0, 7]
    assert abs(res["wea"][0, 0, 0, 0] + res["we"][0, 0, 0, 0]) <= 64 * cc.U * res["we"][0, 0, 0, 0]
    mom = hip.eddington_moments(res)
    assert mom["K_over_J"].shape == (1, 1) and abs(mom["K_over_J"][0, 0] - 1.0) < 1e-13      # streaming: K / J = 1
    closed = e.comoving_field(cc.SHELLS, EVERY_E, np.linspace(-1.0, 1.0, 9), [1.0e12, 1.2e12], [0.9, 1.01])
    invariants(closed, "top edge 1")
    assert closed["count"][0, 0, 0].tolist() == [10, 0, 0, 0, 0, 0, 0, 0] and closed["n_outside"] == 30 and closed["n_observable"] == n
    e.close()


# ---------------------------------------------------------------------------------------------- another context's frame, pools, real frames
def test_frame_of_another_context(hip):
    """the photons' own context holds a slab with a gap; a second context holds the whole frame, where the photons of the gap are located"""
    c = cc.case("gap")
    own = engine_for(hip, c["frame"], c["ph"])
    big = engine_for(hip, c["whole"])
    before = own.get_photons()
    through_slab = own.comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES)
    through_whole = own.comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES, hydro=big)
    after = own.get_photons()
    for k in before:                                       # no photon column changes, the cell index included
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    compare(through_slab, cc.want("gap", cc.CELLS), "own slab")
    compare(through_whole, cc.field(c["whole"], c["ph"], cc.CELLS, cc.E_EDGES, cc.A_EDGES), "the whole frame of another context")
    assert through_whole["count"].shape == (256, 6, 4) and through_slab["count"].shape == (c["frame"]["num_elements"], 6, 4) != (256, 6, 4)
    assert through_whole["n_unlocated"] + 20 < through_slab["n_unlocated"] and through_whole["count"].sum() > through_slab["count"].sum() + 20
    shells = own.comoving_field(cc.SHELLS, cc.E_EDGES, cc.A_EDGES, cc.SHELL_R, cc.SHELL_MU, hydro=big)
    compare(shells, cc.field(c["whole"], c["ph"], cc.SHELLS, cc.E_EDGES, cc.A_EDGES, cc.SHELL_R, cc.SHELL_MU), "SHELLS in the whole frame")
    own.close()
    big.close()


def test_after_a_real_frame(hip):
    """the columns the loop actually leaves behind: 1000 injected photons through one exact-mode frame on the 2-D cylindrical block mesh"""
    frame, ph, cfg = synth.config2(n_photons=1000, nzc=8, stokes=0, lumi=5e51)
    e = engine_for(hip, frame, ph)
    _, st = e.propagate_frame(0.0, 0.5 / frame["fps"], 4242)
    assert st.frame_scatt_cnt > 0
    after = e.get_photons()
    assert not np.array_equal(after["r2"], ph["r2"]) and after["num_scatt"].sum() > 0
    q = cc.per_photon(frame, after)
    at = q["cell"] >= 0
    r_edges, mu_edges = hip.shell_edges(np.linspace(np.percentile(q["r"], 2), np.percentile(q["r"], 98), 7), [0.0, 0.5, 1.0, 1.5, 2.0, 2.5])
    e_edges = 10.0 ** np.linspace(np.log10(np.percentile(q["e"][at], 3)), np.log10(np.percentile(q["e"][at], 97)), 9) * 1.000123
    a_edges = hip.cosine_edges(8)
    res = e.comoving_field(cc.SHELLS, e_edges, a_edges, r_edges, mu_edges)
    want = cc.field(frame, after, cc.SHELLS, e_edges, a_edges, r_edges, mu_edges)
    compare(res, want, "after a frame, SHELLS 6 x 5 x 8 x 8", fragile_ok=True)
    assert want["n_fragile"] <= 2 and res["count"].sum() > 500 and res["n_outside"] > 10
    cells = e.comoving_field(cc.CELLS, e_edges[[0, -1]], a_edges)
    compare(cells, cc.field(frame, after, cc.CELLS, e_edges[[0, -1]], a_edges), "after a frame, CELLS x 1 x 8", fragile_ok=True)
    # the jet streams outwards in the lab (K_lab / J_lab near 1) and is much less beamed in its own frame
    mom = hip.eddington_moments(res)
    used = mom["J"] > 0
    assert used.sum() > 10 and np.isnan(mom["K_over_J"][~used]).all() and np.isfinite(mom["H_over_J_lab"][used]).all()
    assert np.median(mom["K_over_J_lab"][used]) > 0.9 and np.median(mom["K_over_J"][used]) < 0.8
    chk = cc.moments(res)
    for k in chk:
        assert np.array_equal(np.nan_to_num(mom[k], nan=-7.0), np.nan_to_num(chk[k], nan=-7.0)), k
    e.close()


def test_pool_of_three_ragged_lists(hip):
    c = cc.case("shells")
    lens, ranks = [137, 300, 3], [0, 1, 3]                 # rank 2 is never created
    pool = engine_for(hip, c["frame"])
    pool.pool_create(4, 320)
    first, subs = 0, []
    for r, m in zip(ranks, lens):
        subs.append({k: v[first:first + m].copy() for k, v in c["ph"].items()})
        pool.pool_rank(r, r).set_photons(subs[-1])
        first += m
    for mode in (cc.CELLS, cc.SHELLS):
        args = (cc.E_EDGES, cc.A_EDGES) + shells_args(mode)
        res = pool.pool_comoving_field(mode, *args)
        views = [pool.pool_rank(r, r).comoving_field(mode, *args) for r in ranks]
        wants = [cc.field(c["frame"], sub, mode, *args) for sub in subs]
        for r, v, w in zip(ranks, views, wants):
            compare(v, w, "view %d, mode %d" % (r, mode))
        total = cc.add(wants)
        compare(res, total, "pool, mode %d" % mode)
        assert np.array_equal(res["count"], sum(v["count"] for v in views)) and res["n_observable"] == sum(v["n_observable"] for v in views)
        for k in cc.SUMS:                                   # the pool's call equals the per-view calls added up, within the summed bounds
            assert (np.abs(res[k] - sum(v[k] for v in views)) <= 2 * total["bound_" + k]).all(), k
        assert res["count"].sum() > 150
    with pytest.raises(hip.McratHipError, match="mcrat_hip_pool_comoving_field takes the pool"):
        pool.comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES)
    with pytest.raises(hip.McratHipError, match="no rank pool"):
        pool.pool_rank(0, 0).pool_comoving_field(cc.CELLS, cc.E_EDGES, cc.A_EDGES)
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
    a_edges = np.array([-1.0, -0.31, 0.37, np.nextafter(1.0, 2.0)])
    try:
        results = []
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            recs = [pool.get_photons_range(r * stride, lens[r]) for r in range(R)]
            cat = {k: np.concatenate([a[k] for a in recs]) for k in ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "weight", "num_scatt", "type")}
            res = pool.pool_comoving_field(cc.CELLS, EVERY_E, a_edges)
            want = cc.field(frame, cat, cc.CELLS, EVERY_E, a_edges)
            compare(res, want, "pool, frame %d of a captured plan" % f, fragile_ok=True)
            assert want["n_fragile"] <= 1 and res["count"].sum() > 800
            results.append((res, cat))
        assert not np.array_equal(results[0][1]["r2"], results[1][1]["r2"]) and not np.array_equal(results[0][0]["we"], results[1][0]["we"])
    finally:
        pool.pool_select_frame(-1)
        pool.close()


# ---------------------------------------------------------------------------------------------- oracle-free: the radiation field, isotropy
def test_summed_over_energy_and_cosine_it_is_the_radiation_field(hip):
    """edges that cover every energy and every cosine, in 6 x 4 bins: count summed over them is radiation_field's count exactly; w, we / we_comv and
    we_lab agree within the two products' summation bounds added"""
    c = cc.case("shells")
    e = engine_for(hip, c["frame"], c["ph"])
    e_edges = np.concatenate([[0.0], cc.E_EDGES[1:-1], [1e300]])
    a_edges = np.concatenate([cc.A_EDGES[:-1], [2.0]])
    res = e.comoving_field(cc.SHELLS, e_edges, a_edges, cc.SHELL_R, cc.SHELL_MU)
    rad = e.radiation_field(rc.SHELLS, rc.SHELL_R, rc.SHELL_MU)
    e.close()
    invariants(res, "covering edges")
    for k in ("n_observable", "n_unlocated", "n_outside"):
        assert res[k] == rad[k], k
    assert np.array_equal(res["count"].sum(axis=(2, 3)), rad["count"]) and rad["count"].sum() > 300 and (res["count"] > 0).sum() > 100
    rwant = rc.want("shells", rc.SHELLS)
    n = rad["count"].astype(np.float64)
    for k, kr in (("w", "w"), ("we", "we_comv"), ("we_lab", "we_lab")):
        # both kernels' terms are the same bits (the same expressions on the same operands) and all positive: what differs is the order of the
        # sums.  The radiation field's is within (n + 2) u sum|t| of the exact sum; so are the comoving field's 24 bins together (each has at most
        # n terms), and this test's sum over them adds 24 roundings: the two bounds added
        mag = rwant[kr]
        assert (mag >= 0).all() and (np.abs(res[k].sum(axis=(2, 3)) - rad[kr]) <= (2 * (n + 2.0) + 24.0) * cc.U * mag).all(), k


def test_isotropic_radiation_has_eddington_factor_one_third(hip):
    """4096 equal-weight photons drawn isotropically, with one energy, in the frame of the cell they sit in, taken to the lab with the textbook boost
    by -v (Lorentz factors up to 10), binned into one shell, one energy bin and eight cosine bins: the device's H / J and K / J lie within 5 sigma of 0
    and 1 / 3, sigma = 1 / sqrt(3 N) = 0.0090 and sqrt(4 / (45 N)) = 0.0047 for equal weights and energies.  (The definition gives -0.0106 and 0.3284
    for this construction; the same photons measured about the flow in the lab frame give 0.943 and 0.918: a kernel that bins the lab cosine, drops
    the boost or takes another cell's velocity fails by a hundred sigma.)"""
    n = 4096
    iso = cc.isotropic(n)
    e = engine_for(hip, iso["frame"], iso["ph"])
    res = e.comoving_field(cc.SHELLS, [1e-9, 1e-6], hip.cosine_edges(8), [1.0e12, 1.2e12], [0.9, 1.01])
    e.close()
    invariants(res, "isotropic")
    assert res["count"].shape == (1, 1, 1, 8) and res["count"].sum() == n and res["n_outside"] == 0 and res["n_unlocated"] == 0
    mom = hip.eddington_moments(res)
    h, k = float(mom["H_over_J"][0, 0]), float(mom["K_over_J"][0, 0])
    s_h, s_k = 1.0 / np.sqrt(3.0 * n), np.sqrt(4.0 / (45.0 * n))
    print("isotropic in the fluid frame, on the device: H / J = %.4f (sigma %.4f), K / J = %.4f (sigma %.4f); eight cosine bins hold %s"
          % (h, s_h, k, s_k, res["count"].ravel().tolist()))
    assert abs(h) <= 5 * s_h and abs(k - 1.0 / 3.0) <= 5 * s_k
    assert abs(mom["J"][0, 0] / (n * 1.0e49 * 3.1e-8) - 1.0) < 1e-10            # the one energy comes back
    assert (np.abs(res["count"].ravel() - n / 8) < 5 * np.sqrt(n / 8 * 7 / 8)).all()      # flat in a
    assert mom["K_over_J_lab"][0, 0] - 1.0 / 3.0 > 20 * s_k                    # ... and far from isotropic in the lab, about the radial direction too


# ---------------------------------------------------------------------------------------------- refusals and helpers
def test_refusals_reach_the_caller(hip, monkeypatch):
    c = cc.case("cells_n63")
    e = engine_for(hip, c["frame"], c["ph"])
    r, mu, ee, ae = cc.SHELL_R, cc.SHELL_MU, cc.E_EDGES, cc.A_EDGES
    S = cc.SHELLS
    for args, text in (((7, ee, ae), "mode must be MCRAT_HIP_COMOVING_CELLS or MCRAT_HIP_COMOVING_SHELLS"),
                       ((S, ee, ae), "e_edges and a_edges are needed, and SHELLS needs r_edges and mu_edges"),
                       ((cc.CELLS, None, ae), "e_edges and a_edges are needed"),
                       ((cc.CELLS, ee, None), "e_edges and a_edges are needed"),
                       ((S, ee, ae, r[:1], mu), "must each be at least 1"),
                       ((S, ee, ae, r, mu[:1]), "must each be at least 1"),
                       ((cc.CELLS, ee[:1], ae), "must each be at least 1"),
                       ((cc.CELLS, ee, ae[:1]), "must each be at least 1"),
                       ((S, ee, ae, [1e12, np.inf], mu), "r_edges holds a value that is not finite"),
                       ((S, ee, ae, r, [0.5, np.nan, 1.0]), "mu_edges holds a value that is not finite"),
                       ((cc.CELLS, [0.0, np.inf], ae), "e_edges holds a value that is not finite"),
                       ((cc.CELLS, ee, [-1.0, np.nan]), "a_edges holds a value that is not finite"),
                       ((S, ee, ae, r[::-1], mu), "r_edges is not strictly ascending"),
                       ((S, ee, ae, r, [0.5, 0.5, 1.0]), "mu_edges is not strictly ascending"),
                       ((S, ee[::-1], ae, r, mu), "e_edges is not strictly ascending"),
                       ((S, ee, [-1.0, 1.0, 1.0], r, mu), "a_edges is not strictly ascending"),
                       ((S, ee, [0.0, np.nan], [1.0, 1.0], mu), "a_edges holds a value that is not finite"),      # every axis finite before any ascending
                       ((S, [0.0, 0.0], [0.0, 0.0], r, [0.5, 0.5, 1.0]), "mu_edges is not strictly ascending"),      # ... in the axis order
                       ((S, np.arange(10240.0), ae, r[:2], mu[:2]), "the edges do not fit the kernel's LDS budget"),
                       ((cc.CELLS, np.arange(4201.0), np.arange(2001.0)), "overflows an int")):      # 256 cells x 4200 x 2000: once the frame is known
        with pytest.raises(hip.McratHipError, match=text):
            e.comoving_field(*args)
    edge = np.zeros(1)
    ptr = edge.ctypes.data_as(hip._dp)
    bins = hip.ComovingBins(S, 256, ptr, 256, ptr, 256, ptr, 128, ptr)         # 2^31 bins: refused before the arrays are looked at
    n_bins = hip.C.c_int(0)
    assert e.lib.mcrat_hip_comoving_field_bins(e.ctx, None, hip.C.byref(bins), hip.C.byref(n_bins)) == -1
    assert b"overflows an int" in e.lib.mcrat_hip_last_error(e.ctx)
    monkeypatch.setenv("MCRAT_HIP_COMOVING_PATH", "hbm")
    with pytest.raises(hip.McratHipError, match="MCRAT_HIP_COMOVING_PATH must be lds or global"):
        e.comoving_field(cc.CELLS, ee, ae)
    with pytest.raises(hip.McratHipError, match="a_edges is not strictly ascending"):      # the arguments come before the switch
        e.comoving_field(S, ee, ae[::-1], r, mu)
    monkeypatch.setenv("MCRAT_HIP_COMOVING_PATH", "lds")
    with pytest.raises(hip.McratHipError, match="CELLS always accumulates in global memory"):
        e.comoving_field(cc.CELLS, ee, ae)
    with pytest.raises(hip.McratHipError, match="the planes do not fit the kernel's LDS budget"):
        e.comoving_field(S, np.arange(1138.0), [-1.0, 2.0], [1e12, 1.2e12], [0.0, 1.0])
    monkeypatch.delenv("MCRAT_HIP_COMOVING_PATH")
    other = hip.Engine(synth.TWO, synth.CARTESIAN, 0)                    # a frame on a context with other switches
    other.set_hydro(dict(c["frame"], geometry=synth.CARTESIAN))
    with pytest.raises(hip.McratHipError, match="comoving_field: a frame staged on a context with other switches"):
        e.comoving_field(cc.CELLS, ee, ae, hydro=other)
    with pytest.raises(hip.McratHipError, match="mode must be"):           # ... and the arguments come before the frame
        e.comoving_field(9, ee, ae, hydro=other)
    bare = hip.Engine(*CYL, 0)
    with pytest.raises(hip.McratHipError, match="comoving_field: no staged hydro frame"):
        e.comoving_field(cc.CELLS, ee, ae, hydro=bare)
    no_photons = engine_for(hip, c["frame"])
    with pytest.raises(hip.McratHipError, match="comoving_field: no photons"):
        no_photons.comoving_field(cc.CELLS, ee, ae)
    compare(e.comoving_field(cc.CELLS, ee, ae), cc.want("cells_n63", cc.CELLS), "the context still works")
    for x in (other, bare, no_photons, e):
        x.close()


def test_cosine_edges_and_eddington_moments_follow_their_definitions(hip):
    a = hip.cosine_edges(4)
    assert a.tolist() == [-1.0, -0.5, 0.0, 0.5, np.nextafter(1.0, 2.0)]
    assert hip.cosine_edges(1).tolist() == [-1.0, np.nextafter(1.0, 2.0)]
    res = {"we": np.array([[[1.0, 3.0]], [[0.0, 0.0]]]), "wea": np.array([[[-0.5, 1.5]], [[0.0, 0.0]]]), "weaa": np.array([[[0.25, 0.75]], [[0.0, 0.0]]]),
           "we_lab": np.array([[[2.0, 6.0]], [[1.0, 0.0]]]), "wem": np.array([[[2.0, 6.0]], [[-1.0, 0.0]]]), "wemm": np.array([[[2.0, 6.0]], [[1.0, 0.0]]])}
    mom = hip.eddington_moments(res)
    assert mom["J"].tolist() == [4.0, 0.0] and mom["H"].tolist() == [1.0, 0.0] and mom["K"].tolist() == [1.0, 0.0]
    assert mom["K_over_J"][0] == 0.25 and mom["H_over_J"][0] == 0.25 and np.isnan(mom["K_over_J"][1]) and np.isnan(mom["H_over_J"][1])
    assert mom["J_lab"].tolist() == [8.0, 1.0] and mom["K_over_J_lab"].tolist() == [1.0, 1.0] and mom["H_over_J_lab"].tolist() == [1.0, -1.0]
