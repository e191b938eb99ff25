"""Photon birth on the device in EVERY (DIMENSIONS, GEOMETRY) pair: the injection (mcrat_hip_inject_photons, mcrat_hip_pool_inject_photons), the
cyclo-synchrotron pool emission, and the replacement of a scattered pool photon inside the loop -- the hook of mcrat.c:786-808 in the CSH builds of
rank_loop_kernel (64 / 128 / 256 threads per list) and as cs_replace*_kernel between launches.  All of it branches on the pair: the slab test, the cell
volume, hydro -> MCRaT coordinates, the cell's velocity at the photon's azimuth, the B-field magnitude.

Two kinds of check, on the frames of tests.test_gpu_instantiations._case:
  * parity with the oracle, asserted as the tests that cover a few pairs assert it (test_photon_injection_equals_oracle,
    test_pool_emission_matches_the_oracle, test_scatter_frame_with_the_switch_on_matches_the_oracle,
    test_pool_lists_with_the_switch_on_match_the_oracle_list_by_list): integers exact, doubles 1e-11 at birth and 1e-9 after a frame;
  * the oracle-free invariants of tests/birth_checker.py on the device's own photons (the oracle restates the same reference lines by the same hand: a
    geometry mistake common to both passes every parity test), and Engine.lookup_cell against the brute-force cell.

The slab is laid around the case's own photons (birth_checker.slab_around).  The figures each invariant looked at are printed (pytest -rP)."""
import functools

import numpy as np
import pytest

from mcrat_amd import synth
from tests import birth_checker as B
from tests.test_gpu_cyclosynch import _oracle_pool
from tests.test_gpu_instantiations import GEOMS, NAMES, PAIRS, _case
from tests.test_gpu_pool_cyclosynch import _oracle_frame, _start_list

pytestmark = pytest.mark.gpu

PAIR_IDS = ["%s-%s" % (NAMES[d], GEOMS[g]) for d, g in PAIRS]
WEIGHT, MIN_PHOTONS, MAX_PHOTONS, SEED = 1e42, 2000, 6000, 2024
# the pairs tests/test_gpu_cyclosynch.py's CS_FRAMES does not run
NEW_CS_PAIRS = [(synth.TWO, synth.CARTESIAN), (synth.TWO, synth.SPHERICAL), (synth.TWO_POINT_FIVE, synth.CARTESIAN),
                (synth.TWO_POINT_FIVE, synth.CYLINDRICAL), (synth.TWO_POINT_FIVE, synth.SPHERICAL), (synth.THREE, synth.POLAR)]
CS_MAX_PHOTONS = 2000


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


# ------------------------------------------------------------------ injection
@pytest.mark.parametrize("spect", ["b", "w"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_injection_in_every_geometry(hip, oracle, pair, spect):
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, 0)
    args = dict(B.slab_around(ph), spect=spect)
    ref, wref = oracle.photon_injection(oracle.make_config(dims, geom, 0), oracle.OracleHydro(frame), args["r_inj"], WEIGHT, MIN_PHOTONS, MAX_PHOTONS, spect,
                                        args["theta_min"], args["theta_max"], seed=SEED)
    e = hip.Engine(dims, geom, 0)
    e.set_hydro(frame)
    n, w = e.inject_photons(args["r_inj"], WEIGHT, MIN_PHOTONS, MAX_PHOTONS, spect, args["theta_min"], args["theta_max"], frame["fps"], SEED)
    assert n == len(ref) and MIN_PHOTONS <= n <= MAX_PHOTONS and w == wref
    out = e.get_photons_aos()
    for k in ("type", "num_scatt", "weight", "nearest_block_index", "recalc_properties", "s0", "s1", "s2", "s3"):
        assert np.array_equal(out[k], ref[k]), k
    for k in ("r0", "r1", "r2", "p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        scale = np.abs(ref[k])
        if k in ("p1", "p2", "p3"):
            scale = np.abs(ref["p0"])
        if k in ("comv_p1", "comv_p2", "comv_p3"):
            scale = np.abs(ref["comv_p0"])
        if k in ("r0", "r1", "r2"):
            scale = np.maximum(scale, 1e9)
        assert (np.abs(out[k] - ref[k]) <= 1e-11 * scale).all(), k
    # the injected photons run: every pass locates every one of them
    e.begin_frame(5, 0.0, 1.0 / frame["fps"])
    st = e.run(3)
    assert st.iterations == 3 and st.not_found == 0
    assert (e.get_photons()["nearest_block_index"] >= 0).all()
    # the invariants, on the photons as the device made them
    rep = B.check_injection(frame, cfg, out, w, args)
    print("%s %s: %s" % (PAIR_IDS[PAIRS.index(pair)], spect, B.figures(rep)))
    # the device's cell search puts each of them where the brute-force scan does
    a0, a1, a2 = rep["hydro"]
    got = e.lookup_cell(a0, a1, a2 if dims == synth.THREE else None)
    e.close()
    assert np.array_equal(got, rep["cell"])


@pytest.mark.parametrize("pair", [(synth.TWO, synth.CARTESIAN), (synth.TWO_POINT_FIVE, synth.CYLINDRICAL), (synth.THREE, synth.POLAR)],
                         ids=["2d-cartesian", "2.5d-cylindrical", "3d-polar"])
def test_pool_injection_in_more_geometries(hip, pair):
    """mcrat_hip_pool_inject_photons against mcrat_hip_inject_photons on the views, as
    test_pool_injection_gives_every_list_the_photons_of_its_own_injection does in 2-D spherical with black bodies"""
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, 1)
    args = B.slab_around(ph)
    fps = frame["fps"]
    common = dict(r_inj=args["r_inj"], theta_min=args["theta_min"], theta_max=args["theta_max"], min_photons=300, max_photons=900)
    specs = [dict(common, ph_weight=1e53, spect="b", seed=11),
             None,
             dict(common, ph_weight=3e52, spect="w", seed=12),
             dict(common, ph_weight=1e44, spect="b", seed=13)]                 # the weight loop has to climb
    R = len(specs)
    pools = []
    for batched in (True, False):
        pool = hip.Engine(dims, geom, 1)
        pool.set_hydro(frame)
        pool.pool_create(R, 1024)
        views = [pool.pool_rank(r, 70 + r) for r in range(R)]
        if batched:
            got = pool.pool_inject_photons(fps, specs)
        else:
            got = [None if q is None else views[r].inject_photons(q["r_inj"], q["ph_weight"], q["min_photons"], q["max_photons"], q["spect"], q["theta_min"],
                                                                  q["theta_max"], fps, q["seed"]) for r, q in enumerate(specs)]
        pools.append((pool, views, got))
    (pa, va, ga), (pb, vb, gb) = pools
    assert ga == gb and ga[1] is None and ga[3][1] > 1e44
    assert len({g[0] for g in ga if g}) >= 2                                  # Poisson-sized lists
    for r, q in enumerate(specs):
        if q is None:
            assert pa.pool_summaries()[r].list_capacity == 0
            continue
        a, b = va[r].get_photons(), vb[r].get_photons()
        assert len(a["p0"]) == ga[r][0] and q["min_photons"] <= ga[r][0] <= q["max_photons"]
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=(np.asarray(a[k]).dtype.kind == "f")), (r, k)
    pa.close()
    pb.close()


# ------------------------------------------------------------------ pool emission
EMISSIONS = [(p, b) for p in PAIRS for b in (0, 1)] + [((synth.TWO_POINT_FIVE, synth.SPHERICAL), 2), ((synth.THREE, synth.POLAR), 2)]


@pytest.mark.parametrize("pair,b_field_calc", EMISSIONS, ids=["%s-field%d" % (PAIR_IDS[PAIRS.index(p)], b) for p, b in EMISSIONS])
def test_pool_emission_in_every_geometry(hip, oracle, pair, b_field_calc):
    """mcrat_hip_emit_cyclosynch_pool against orc_photonEmitCyclosynch as test_pool_emission_matches_the_oracle asserts it (its null-slots case); then
    the invariants on the device's pool photons"""
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, 1)
    args = dict(B.slab_around(ph), scatt_frame_number=200, inj_frame_number=200)
    dens = np.ascontiguousarray(frame["dens"])
    fields = [None, None, None]
    if b_field_calc == 2:
        g = np.random.default_rng(5)
        fields = [np.ascontiguousarray(g.uniform(1e3, 1e5, frame["num_elements"])) for _ in range(3)]
    aos = synth.photons_to_aos(ph, hip.PHOTON_DTYPE)
    n_ref, w_ref, fb_ref, aos, want = _oracle_pool(oracle, frame, cfg, aos, range(1, len(aos), 2), dens, b_field_calc, 77, 1500, B=fields,
                                                   r_inj=args["r_inj"], theta_min=args["theta_min"], theta_max=args["theta_max"])
    e = hip.Engine(dims, geom, 1)
    e.set_hydro(frame)
    e.set_hydro_extras(dens, *fields)
    e.set_photons_aos(aos)
    n, w, bad = e.emit_cyclosynch_pool(args["r_inj"], 1e40, 1500, args["theta_min"], args["theta_max"], frame["fps"], 77, b_field_calc=b_field_calc,
                                       scatt_frame_number=200, inj_frame_number=200)
    assert (n, w, bad) == (n_ref, w_ref, 0) and fb_ref == 0
    assert e.n == len(want)
    got = e.get_photons_aos()
    e.close()
    assert 1 <= n <= 150
    assert np.array_equal(got["type"], want["type"]) and np.array_equal(got["weight"], want["weight"])
    assert np.array_equal(got["nearest_block_index"], want["nearest_block_index"]) and np.array_equal(got["recalc_properties"], want["recalc_properties"])
    pool = got["type"] == b"p"
    assert pool.sum() == n
    for f in ("comv_p0",):
        assert np.allclose(got[f][pool], want[f][pool], rtol=1e-14)
    for f in ("p0", "p1", "p2", "p3", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2"):
        scale = np.abs(want["p0"][pool]) if f.startswith("p") else (np.abs(want["comv_p0"][pool]) if f.startswith("comv") else 1e12)
        assert np.all(np.abs(got[f][pool] - want[f][pool]) <= 1e-11 * scale), f
    rest = ~pool
    for f in ("p0", "r0", "num_scatt", "s0"):
        assert np.array_equal(got[f][rest], want[f][rest], equal_nan=True), f
    new = np.flatnonzero((aos["type"] == b"N") & (got["type"] != b"N"))
    assert len(new) == n
    rep = B.check_pool_emission(frame, cfg, got[new], w, args)
    print("%s field %d: %s" % (PAIR_IDS[PAIRS.index(pair)], b_field_calc, B.figures(rep)))


# ------------------------------------------------------------------ the scatter frame with the switch on
def _cs_case(dims, geom, stokes):
    """the case's frame, its first 300 photons, and the arguments of a scatter frame with the switch on"""
    frame, ph, cfg = _case(dims, geom, stokes)
    args = B.slab_around(ph)
    ph = {k: v[:300] for k, v in ph.items()}
    remaining = 0.02 if (dims, geom) == (synth.TWO, synth.SPHERICAL) else 0.05          # (0.05 s there are 8798 passes, 1.7 s of oracle)
    ang_phi = 45.0 if dims == synth.THREE else 10.0
    return frame, ph, cfg, args, remaining, ang_phi


@functools.lru_cache(maxsize=None)
def _oracle_cs_frame(dims, geom, stokes, shift, seed, stream):
    """one oracle run per (pair, STOKES, list): 300 photons + 300 null slots rolled by `shift`, orc_scatter_frame_cs without a pass cap"""
    from oracle import oracle_py as oracle
    frame, ph, cfg, args, remaining, ang_phi = _cs_case(dims, geom, stokes)
    before = _start_list(oracle, ph, shift)
    want, st, cnt, t = _oracle_frame(oracle, cfg, frame, np.ascontiguousarray(frame["dens"]), [None, None, None], before, seed, stream, remaining,
                                     CS_MAX_PHOTONS, args["theta_max"], 1, 1, ang_phi, r_inj=args["r_inj"], stokes=stokes)
    for a in (before, want):
        a.setflags(write=False)
    return before, want, st, cnt, t


def _compare_cs_list(got, want, what):
    """the list after a frame, as test_scatter_frame_with_the_switch_on_matches_the_oracle compares it"""
    assert len(got) == len(want), what
    assert np.array_equal(got["type"], want["type"]), what
    for f in ("weight", "num_scatt", "nearest_block_index", "recalc_properties"):
        assert np.array_equal(got[f], want[f]), (what, f)
    for f in ("p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2", "s0", "s1", "s2", "s3"):
        scale = np.maximum(np.abs(want["p0"]), 1e-300) if f.startswith("p") else (
            np.maximum(np.abs(want["comv_p0"]), 1e-300) if f.startswith("comv") else (np.maximum(np.abs(want[f]), 1e9) if f.startswith("r") else 1.0))
        err = np.abs(got[f] - want[f]) / scale
        assert np.all(err <= 1e-9), (what, f, float(err.max()), int(err.argmax()))


@pytest.mark.parametrize("stokes", [0, 1], ids=["stokes-off", "stokes-on"])
@pytest.mark.parametrize("pair", NEW_CS_PAIRS, ids=[PAIR_IDS[PAIRS.index(p)] for p in NEW_CS_PAIRS])
def test_scatter_frame_with_the_switch_on_in_more_geometries(hip, oracle, pair, stokes):
    """mcrat_hip_scatter_frame_cyclosynch (one list) against orc_scatter_frame_cs: pool emission, the loop with its replacements and the list's
    doubling, the absorption at the end; counters exact, doubles 1e-9"""
    dims, geom = pair
    frame, ph, cfg, args, remaining, ang_phi = _cs_case(dims, geom, stokes)
    before, want, st, cnt, t = _oracle_cs_frame(dims, geom, stokes, 0, 31, 0)
    assert len(want) > 600 and cnt.scatt_cyclosynch_num_ph > 30 and cnt.frame_abs_cnt > 100 and cnt.rebins == 0
    e = hip.Engine(dims, geom, stokes, cyclosynchrotron=1)
    e.set_hydro(frame)
    e.set_hydro_extras(np.ascontiguousarray(frame["dens"]), None, None, None)
    e.set_photons_aos(before.astype(hip.PHOTON_DTYPE))
    tn, gst, gcnt = e.scatter_frame_cyclosynch(0.0, remaining, 31, args["r_inj"], 1e40, CS_MAX_PHOTONS, 0.0, args["theta_max"], frame["fps"], emit_pool=1,
                                               max_iterations=0, b_field_calc=1, rebin_ang_phi=ang_phi, scatt_frame_number=200, inj_frame_number=200)
    got = e.get_photons_aos()
    e.close()
    assert (gst.iterations, gst.frame_scatt_cnt, gst.kn_rejections) == (st.iterations, st.frame_scatt_cnt, st.kn_rejections)
    assert (gcnt.num_cyclosynch_ph_emit, gcnt.scatt_cyclosynch_num_ph, gcnt.frame_abs_cnt, gcnt.rebins) == \
        (cnt.num_cyclosynch_ph_emit, cnt.scatt_cyclosynch_num_ph, cnt.frame_abs_cnt, cnt.rebins)
    assert gcnt.pool_weight == cnt.pool_weight and gcnt.n_comptonized == pytest.approx(cnt.n_comptonized, rel=1e-12)
    assert tn == pytest.approx(t, rel=1e-12)
    _compare_cs_list(got, want, PAIR_IDS[PAIRS.index(pair)])


# ------------------------------------------------------------------ the hook builds of the loop kernel
HOOK_LISTS = [(0, 31), (7, 41)]            # (roll, seed) per list, as _start_list and POOLS lay lists out


def _run_hook_pool(hip, dims, geom, stokes):
    frame, ph, cfg, args, remaining, ang_phi = _cs_case(dims, geom, stokes)
    pool = hip.Engine(dims, geom, stokes, cyclosynchrotron=1)
    pool.set_hydro(frame)
    pool.set_hydro_extras(np.ascontiguousarray(frame["dens"]), None, None, None)
    pool.pool_create(len(HOOK_LISTS), 4800)                  # 600 slots to start with, room for three doublings
    largs = []
    for r, (shift, seed) in enumerate(HOOK_LISTS):
        before = _oracle_cs_frame(dims, geom, stokes, shift, seed, r)[0]
        pool.pool_rank(r, r).set_photons_aos(before.astype(hip.PHOTON_DTYPE))
        largs.append(dict(seed=seed, time_now=0.0, remaining_time=remaining, r_inj=args["r_inj"], ph_weight_suggest=1e40, theta_min=0.0,
                          theta_max=args["theta_max"], emit_pool=1, scatt_frame_number=200, inj_frame_number=200))
    sts, cnts = pool.pool_scatter_frames_cyclosynch(largs, CS_MAX_PHOTONS, frame["fps"], b_field_calc=1, rebin_ang_phi=ang_phi)
    lists = [pool.pool_rank(r, r).get_photons_aos() for r in range(len(HOOK_LISTS))]
    pool.close()
    return sts, cnts, lists


@pytest.mark.parametrize("threads", ["64", "128", "256"])
@pytest.mark.parametrize("stokes", [0, 1], ids=["stokes-off", "stokes-on"])
@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_every_hook_build_of_the_loop_kernel_equals_the_oracle(hip, oracle, pair, stokes, threads, monkeypatch):
    """every CSH instantiation of rank_loop_kernel -- nine pairs x STOKES x 64 / 128 / 256 threads per list -- through
    mcrat_hip_pool_scatter_frames_cyclosynch, list by list against orc_scatter_frame_cs as
    test_pool_lists_with_the_switch_on_match_the_oracle_list_by_list asserts it"""
    dims, geom = pair
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", threads)
    monkeypatch.delenv("MCRAT_HIP_CS_HOOK_KERNEL", raising=False)
    sts, cnts, lists = _run_hook_pool(hip, dims, geom, stokes)
    grew = 0
    for r, (shift, seed) in enumerate(HOOK_LISTS):
        before, want, st, cnt, t = _oracle_cs_frame(dims, geom, stokes, shift, seed, r)
        what = (PAIR_IDS[PAIRS.index(pair)], stokes, threads, r)
        g, gc = sts[r], cnts[r]
        assert (g.iterations, g.frame_scatt_cnt, g.kn_rejections) == (st.iterations, st.frame_scatt_cnt, st.kn_rejections), what
        assert (gc.num_cyclosynch_ph_emit, gc.scatt_cyclosynch_num_ph, gc.frame_abs_cnt, gc.rebins) == \
            (cnt.num_cyclosynch_ph_emit, cnt.scatt_cyclosynch_num_ph, cnt.frame_abs_cnt, cnt.rebins), what
        assert gc.pool_weight == cnt.pool_weight and gc.n_comptonized == pytest.approx(cnt.n_comptonized, rel=1e-12)
        assert g.time_now == pytest.approx(t, rel=1e-12) and g.remaining_time == 0.0
        _compare_cs_list(lists[r], want, what)
        grew += len(want) > 600
        assert st.frame_scatt_cnt > 500 and cnt.scatt_cyclosynch_num_ph > 0 and cnt.frame_abs_cnt > 0
    assert grew >= 1                                         # at least one list doubled inside the loop, in its window of the pool


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_the_hook_as_a_kernel_gives_the_same_lists_in_every_geometry(hip, oracle, pair, monkeypatch):
    """MCRAT_HIP_CS_HOOK_KERNEL=1 (cs_replace_pool_kernel between two launches of the loop) against the hook inside the loop kernel: to the byte"""
    dims, geom = pair
    monkeypatch.delenv("MCRAT_HIP_RANK_BLOCK", raising=False)
    runs = {}
    for hook_kernel in ("0", "1"):
        monkeypatch.setenv("MCRAT_HIP_CS_HOOK_KERNEL", hook_kernel)
        runs[hook_kernel] = _run_hook_pool(hip, dims, geom, 1)
    (sa, ca, la), (sb, cb, lb) = runs["0"], runs["1"]
    for r in range(len(HOOK_LISTS)):
        assert (sa[r].iterations, sa[r].frame_scatt_cnt) == (sb[r].iterations, sb[r].frame_scatt_cnt), r
        assert (ca[r].num_cyclosynch_ph_emit, ca[r].scatt_cyclosynch_num_ph, ca[r].frame_abs_cnt, ca[r].rebins) == \
            (cb[r].num_cyclosynch_ph_emit, cb[r].scatt_cyclosynch_num_ph, cb[r].frame_abs_cnt, cb[r].rebins), r
        assert ca[r].scatt_cyclosynch_num_ph > 0
        assert len(la[r]) == len(lb[r]) and la[r].tobytes() == lb[r].tobytes(), r
