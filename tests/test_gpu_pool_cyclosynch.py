"""CYCLOSYNCHROTRON_SWITCH on inside the rank pool (mcrat_hip_pool_scatter_frames_cyclosynch): several lists of one pool go through the
scatter frame of mcrat.c:706-878 in the same launches -- pool emission, the loop in which a scattered pool photon becomes a comptonised
one and is replaced (the list doubling inside its window of the pool), the rebinning trigger, rebinning and absorption -- and every
list must come out as orc_scatter_frame_cs leaves it when run on that list alone: same passes, scatterings, counters, list length,
types, slots and weights; doubles to 1e-9.  The frame is a sequence of steps in engine.hip (pcs_collect, pool_emit_cyclosynch, pcs_upload_hooks,
pcs_choose_block, pcs_loop, pcs_close_counters, pcs_end_rebin, pcs_absorb); the rules it shares with the one-list path -- histogram axes, refusals,
shell radii, weight search -- are list_plan.hpp's (tests/test_list_plan_cpu.py).  Both A/B forms are held equal to the default to the byte:
MCRAT_HIP_POOL_REBIN_EACH=1 (rebinning list by list) and MCRAT_HIP_CS_HOOK_KERNEL=1 (the hook as a kernel between two launches)."""
import ctypes as C

import numpy as np
import pytest

from mcrat_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _oracle_frame(oracle, cfg, frame, dens, B, before, seed, stream, remaining, max_photons, theta_max, emit_pool, b_field_calc, ang_phi, r_inj=1e12, stokes=1):
    L = oracle.lib()
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], stokes)
    H = oracle.OracleHydro(frame)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
    cs = oracle.CS(b_field_calc, 0.5, 0.1, ptr(dens), ptr(B[0]), ptr(B[1]), ptr(B[2]), 200, 200, 0.5, ang_phi)
    l = oracle.PhotonList()
    L.orc_list_init(C.byref(l))
    # as tests/test_gpu_cyclosynch.py builds its list: every slot a photon first (setPhotonList counts all of them in num_photons), then the
    # null slots by setNullPhoton, so that the list's counters are consistent (verifyPhotonNum)
    nulls = np.flatnonzero(before["type"] == b"N")
    full = before.copy()
    full[nulls] = before[0]
    assert L.orc_list_set(C.byref(l), full.ctypes.data, len(full)) == 0
    for i in nulls:
        assert L.orc_list_set_null(C.byref(l), int(i)) == 0
    rng = oracle.Rng()
    L.orc_rng_init(C.byref(rng), seed, stream)
    st, cnt, t = oracle.Stats(), oracle.CSCounts(), C.c_double(0.0)
    L.orc_scatter_frame_cs(C.byref(c), C.byref(cs), C.byref(l), C.byref(H.c), C.byref(rng), C.byref(t), remaining, r_inj, 1e40, max_photons, 0.0, theta_max,
                           emit_pool, 0, C.byref(st), C.byref(cnt))
    assert cnt.error == 0
    buf = (C.c_char * (l.list_capacity * oracle.PHOTON_DTYPE.itemsize)).from_address(l.photons)
    want = np.frombuffer(buf, dtype=oracle.PHOTON_DTYPE).copy()
    L.orc_list_free(C.byref(l))
    return want, st, cnt, t.value


def _start_list(oracle, ph, shift):
    """300 photons + 300 null slots, as tests/test_gpu_cyclosynch.py sets its lists up; `shift` rotates the photons so that the lists differ"""
    aos = np.roll(synth.photons_to_aos(ph, oracle.PHOTON_DTYPE), shift)
    L = oracle.lib()
    l = oracle.PhotonList()
    L.orc_list_init(C.byref(l))
    both = np.concatenate([aos, aos])
    assert L.orc_list_set(C.byref(l), both.ctypes.data, len(both)) == 0
    for i in range(300, 600):
        assert L.orc_list_set_null(C.byref(l), i) == 0
    buf = (C.c_char * (l.list_capacity * oracle.PHOTON_DTYPE.itemsize)).from_address(l.photons)
    before = np.frombuffer(buf, dtype=oracle.PHOTON_DTYPE).copy()
    L.orc_list_free(C.byref(l))
    return before


POOLS = {
    # mesh, B_FIELD_CALC, max_photons, theta_max, rebin_ang_phi, per list: (seed, remaining_time, emit_pool)
    "2d-rebinning-lists": ("2d", 1, 200, 0.05, 10.0, [(31, 3.0, 1), (32, 1.0, 1), (33, 0.7, 0), None, (35, 0.05, 1)]),
    "3d-growing-lists": ("3d", 1, 2000, 0.06, 45.0, [(31, 0.2, 1), (41, 0.2, 1), (42, 0.1, 0)]),
    # BASELINE.json configs[4]'s switches at test size: THREE / SPHERICAL, B_FIELD_CALC == SIMULATION, STOKES on
    "3d-spherical-simulation-field": ("3ds", 2, 2000, 0.2, 45.0, [(31, 0.2, 1), (51, 0.15, 1)]),
}


@pytest.mark.parametrize("threads", ["256", "128", "64"])
@pytest.mark.parametrize("case", sorted(POOLS))
def test_pool_lists_with_the_switch_on_match_the_oracle_list_by_list(hip, oracle, case, threads, monkeypatch):
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", threads)           # large pools run 128-thread lists (four per CU), very large ones 64-thread lists (eight): all builds of the kernel
    mesh, b_field_calc, max_photons, theta_max, ang_phi, lists = POOLS[case]
    if mesh == "2d":
        frame, ph, cfg = synth.config2(n_photons=300, nzc=8, lumi=3e53)
    elif mesh == "3d":
        frame, ph, cfg = synth.config_3d_cartesian(n_photons=300, n=(8, 8, 8))
    else:
        frame, ph, cfg = synth.config_3d(synth.SPHERICAL, n_photons=300)
    dens = np.ascontiguousarray(frame["dens"])
    B = [None, None, None]
    if b_field_calc == 2:
        g = np.random.default_rng(5)
        B = [np.ascontiguousarray(g.uniform(1e3, 1e5, frame["num_elements"])) for _ in range(3)]
    R = len(lists)
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
    pool.set_hydro(frame)
    pool.set_hydro_extras(dens, *B)
    pool.pool_create(R, 4800)                              # 600 slots to start with, room for three doublings
    starts, args = [], []
    for r, spec in enumerate(lists):
        if spec is None:
            starts.append(None); args.append(None)
            continue
        seed, remaining, emit_pool = spec
        before = _start_list(oracle, ph, 7 * r)
        starts.append(before)
        pool.pool_rank(r, r).set_photons_aos(before.astype(hip.PHOTON_DTYPE))
        args.append(dict(seed=seed, time_now=0.0, remaining_time=remaining, r_inj=1e12, ph_weight_suggest=1e40, theta_min=0.0, theta_max=theta_max,
                         emit_pool=emit_pool, scatt_frame_number=200, inj_frame_number=200))
    with pytest.raises(hip.McratHipError):
        pool.run(0)                                        # the plain loop has no hook: refused with the switch on
    sts, cnts = pool.pool_scatter_frames_cyclosynch(args, max_photons, frame["fps"], b_field_calc=b_field_calc, rebin_ang_phi=ang_phi)
    grew = rebinned = 0
    for r, spec in enumerate(lists):
        if spec is None:
            assert cnts[r].num_cyclosynch_ph_emit == 0 and sts[r].iterations == 0
            continue
        seed, remaining, emit_pool = spec
        want, st, cnt, t = _oracle_frame(oracle, cfg, frame, dens, B, starts[r], seed, r, remaining, max_photons, theta_max, emit_pool, b_field_calc, ang_phi)
        g, gc = sts[r], cnts[r]
        assert (g.iterations, g.frame_scatt_cnt, g.kn_rejections) == (st.iterations, st.frame_scatt_cnt, st.kn_rejections), (case, r)
        assert (gc.num_cyclosynch_ph_emit, gc.scatt_cyclosynch_num_ph, gc.frame_abs_cnt, gc.rebins) == \
            (cnt.num_cyclosynch_ph_emit, cnt.scatt_cyclosynch_num_ph, cnt.frame_abs_cnt, cnt.rebins), (case, r)
        assert gc.pool_weight == cnt.pool_weight and gc.n_comptonized == pytest.approx(cnt.n_comptonized, rel=1e-12)
        assert g.time_now == pytest.approx(t, rel=1e-12) and g.remaining_time == 0.0
        got = pool.pool_rank(r, r).get_photons_aos()
        assert len(got) == len(want), (case, r)
        assert np.array_equal(got["type"], want["type"])
        for f in ("weight", "num_scatt", "nearest_block_index", "recalc_properties"):
            assert np.array_equal(got[f], want[f]), (r, f)
        for f in ("p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3", "r0", "r1", "r2", "s0", "s1", "s2", "s3"):
            scale = np.maximum(np.abs(want["p0"]), 1e-300) if f.startswith("p") else (
                np.maximum(np.abs(want["comv_p0"]), 1e-300) if f.startswith("comv") else (np.maximum(np.abs(want[f]), 1e9) if f.startswith("r") else 1.0))
            err = np.abs(got[f] - want[f]) / scale
            assert np.all(err <= 1e-9), (r, f, float(err.max()), int(err.argmax()))
        grew += len(want) > 600
        rebinned += cnt.rebins
        assert st.frame_scatt_cnt > (100 if remaining >= 0.1 else 0)
    assert grew >= 1                                        # at least one list doubled inside the loop, in its window of the pool
    if case == "2d-rebinning-lists":
        assert rebinned >= 1                                # ... and the rebinning trigger parked a list for the host at least once
    pool.close()


# The side exits of cs_emit_pool_kernel and of pool_emit_cyclosynch (engine.hip).  The batched emission is reached through the whole frame only, so the
# frame gets a remaining time in which no photon moves by a bit (3e-20 cm) and nothing scatters; what the frame still does after the emission is the
# absorption that closes it (every pool photon becomes a null slot again), which the one-list side repeats on its view.  Weights: found on the CPU with
# orc_photonEmitCyclosynch on this mesh (seed 31, stream 0) -- the count's mean times the weight is 1.94e46, the first attempt is accepted in every case:
# 3.88e42 gives 5099 photons (mean 5000: 10 sigma = 707 inside 4096 .. 6000), 2.58e43 gives 751 (inside 601 .. 899), 1.29e44 gives 150.
SIDE_EXITS = {
    # max_photons (rebin_e_perc = 0.1 of it bounds the emission), slots per list, per list: (photons, null slots, ph_weight_suggest, theta_min, theta_max)
    "table-overflow": (60000, 6600, [(300, 6300, 3.88e42, 0.0, 0.05), (300, 300, 1.29e44, 0.0, 0.05)]),   # list 0: more than CS_POOL_EMIT_CAP = 4096 photons, error 4
    "no-null-slot-doubles": (2000, 4800, [(300, 0, 1.29e44, 0.0, 0.05)]),                                # the list doubles inside its window, in the kernel
    "no-null-slot-refused": (20000, 4800, [(300, 0, 2.58e43, 0.0, 0.05)]),                               # list_capacity_grown(300, 751) = 600: 300 null slots for 751 photons
    "empty-shell": (2000, 4800, [(300, 300, 1e40, 3.0, 3.1)]),                                          # no cell in the angle range
}
STILL = 1e-30


def _last_error(e):
    return e.lib.mcrat_hip_last_error(e.ctx).decode()


@pytest.mark.parametrize("case", sorted(SIDE_EXITS))
def test_pool_emission_side_exits_equal_the_one_list_emission_on_a_view(hip, oracle, case):
    max_photons, slots, lists = SIDE_EXITS[case]
    frame, ph, cfg = synth.config2(n_photons=300, nzc=8, lumi=3e53)
    dens = np.ascontiguousarray(frame["dens"])
    R = len(lists)
    starts = []
    for r, (n_ph, n_null, w, tmin, tmax) in enumerate(lists):
        aos = np.roll(synth.photons_to_aos(ph, oracle.PHOTON_DTYPE), 7 * r)[:n_ph]
        L, l = oracle.lib(), oracle.PhotonList()                            # (as _start_list: the null slots as setNullPhoton leaves them)
        L.orc_list_init(C.byref(l))
        full = np.concatenate([aos, np.repeat(aos[:1], n_null)])
        assert L.orc_list_set(C.byref(l), full.ctypes.data, len(full)) == 0
        for i in range(n_ph, n_ph + n_null):
            assert L.orc_list_set_null(C.byref(l), i) == 0
        buf = (C.c_char * (l.list_capacity * oracle.PHOTON_DTYPE.itemsize)).from_address(l.photons)
        starts.append(np.frombuffer(buf, dtype=oracle.PHOTON_DTYPE).copy().astype(hip.PHOTON_DTYPE))
        L.orc_list_free(C.byref(l))
    pools = []
    for batched in (True, False):
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
        pool.set_hydro(frame)
        pool.set_hydro_extras(dens, None, None, None)
        pool.pool_create(R, slots)
        for r in range(R):
            pool.pool_rank(r, r).set_photons_aos(starts[r])
        pools.append(pool)
    pa, pb = pools
    args = [dict(seed=31 + r, time_now=0.0, remaining_time=STILL, r_inj=1e12, ph_weight_suggest=w, theta_min=tmin, theta_max=tmax, emit_pool=1,
                 scatt_frame_number=200, inj_frame_number=200) for r, (n_ph, n_null, w, tmin, tmax) in enumerate(lists)]
    got_a, got_b, text_a, text_b = None, [], "", ""
    try:
        sts, cnts = pa.pool_scatter_frames_cyclosynch(args, max_photons, frame["fps"], b_field_calc=1)
        got_a = [(cnts[r].num_cyclosynch_ph_emit, cnts[r].pool_weight, cnts[r].integrals_not_converged) for r in range(R)]
    except hip.McratHipError:
        text_a = _last_error(pa)
    before_b = []
    for r, a in enumerate(args):
        v = pb.pool_rank(r, r)
        before_b.append(v.get_photons_aos())
        try:
            got_b.append(v.emit_cyclosynch_pool(a["r_inj"], a["ph_weight_suggest"], max_photons, a["theta_min"], a["theta_max"], frame["fps"], a["seed"],
                                                b_field_calc=1, scatt_frame_number=200, inj_frame_number=200))
            if got_b[-1][0] > 0:
                v.absorb_cyclosynch(b_field_calc=1)                        # what closes the frame of a list that emitted
        except hip.McratHipError:
            text_b = _last_error(v)
    print(case, got_a, got_b, repr(text_a), repr(text_b))
    assert text_a == text_b
    if case == "no-null-slot-refused":
        assert "fewer null slots than photons to add" in text_a and got_a is None and got_b == []
    else:
        assert text_a == "" and got_a == got_b
        for r in range(R):
            a, b = pa.pool_rank(r, r).get_photons_aos(), pb.pool_rank(r, r).get_photons_aos()
            assert len(a) == len(b), r
            # every column but the loop's own: the frame's one pass has located the photons, filled in their comoving four-momenta and drawn their
            # free paths (nearest_block_index, recalc_properties, comv_p0-3, the optical-depth columns); the emission alone has not
            for f in ("type", "weight", "num_scatt", "p0", "p1", "p2", "p3", "r0", "r1", "r2", "s0", "s1", "s2", "s3"):
                assert np.array_equal(a[f], b[f], equal_nan=(a[f].dtype.kind == "f")), (r, f)
    n0, w0 = (got_b[0][0], got_b[0][1]) if got_b else (None, None)
    if case == "table-overflow":
        assert 4096 < n0 <= 6000 and 1 <= got_b[1][0] <= 200 and (w0, got_b[1][1]) == (lists[0][2], lists[1][2])
    elif case == "no-null-slot-doubles":
        assert 1 <= n0 < 300 and len(pb.pool_rank(0, 0).get_photons_aos()) == 600
    elif case == "empty-shell":
        assert (n0, w0) == (0, lists[0][2])
        assert pb.pool_rank(0, 0).get_photons_aos().tobytes() == before_b[0].tobytes()        # the list untouched
    pa.close()
    pb.close()


def test_dozens_of_lists_rebinned_in_the_same_frame(hip, oracle, monkeypatch):
    """mc_cyclosynch.c:610-710 for all parked lists of a frame in two launches (engine.hip, pool_rebin_lists; inject.hip, rebin_pool_kernel):
    96 lists, of which more than 64 have their rebinning trigger (mcrat.c:797-808) fire in the same frame, come out bit for bit as when every list is rebinned on its own
    through its view (MCRAT_HIP_POOL_REBIN_EACH=1, the round-2 path), and as the oracle leaves them (three of them checked, 1e-9)."""
    frame, ph, cfg = synth.config2(n_photons=300, nzc=8, lumi=3e53)
    dens = np.ascontiguousarray(frame["dens"])
    R, max_photons, theta_max = 96, 200, 0.05
    starts = [_start_list(oracle, ph, 7 * r) for r in range(R)]
    args = [dict(seed=31 + 3 * r, time_now=0.0, remaining_time=8.0 + 0.01 * (r % 7), r_inj=1e12, ph_weight_suggest=1e40, theta_min=0.0, theta_max=theta_max,
                 emit_pool=1, scatt_frame_number=200, inj_frame_number=200) for r in range(R)]
    runs = {}
    for each in ("0", "1"):
        monkeypatch.setenv("MCRAT_HIP_POOL_REBIN_EACH", each)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
        pool.set_hydro(frame)
        pool.set_hydro_extras(dens, None, None, None)
        pool.pool_create(R, 4800)
        for r in range(R):
            pool.pool_rank(r, r).set_photons_aos(starts[r].astype(hip.PHOTON_DTYPE))
        sts, cnts = pool.pool_scatter_frames_cyclosynch(args, max_photons, frame["fps"], b_field_calc=1, rebin_ang_phi=10.0)
        runs[each] = (sts, cnts, [pool.pool_rank(r, r).get_photons_aos() for r in range(R)])
        pool.close()
    (sa, ca, la), (sb, cb, lb) = runs["0"], runs["1"]
    assert sum(1 for r in range(R) if ca[r].rebins >= 1) >= 64
    for r in range(R):
        assert (sa[r].iterations, sa[r].frame_scatt_cnt) == (sb[r].iterations, sb[r].frame_scatt_cnt), r
        assert (ca[r].num_cyclosynch_ph_emit, ca[r].scatt_cyclosynch_num_ph, ca[r].frame_abs_cnt, ca[r].rebins) == \
            (cb[r].num_cyclosynch_ph_emit, cb[r].scatt_cyclosynch_num_ph, cb[r].frame_abs_cnt, cb[r].rebins), r
        assert la[r].tobytes() == lb[r].tobytes(), r
    for r in (0, 35, 95):
        want, st, cnt, t = _oracle_frame(oracle, cfg, frame, dens, [None, None, None], starts[r], args[r]["seed"], r, args[r]["remaining_time"], max_photons,
                                         theta_max, 1, 1, 10.0)
        assert (sa[r].iterations, sa[r].frame_scatt_cnt) == (st.iterations, st.frame_scatt_cnt), r
        assert (ca[r].num_cyclosynch_ph_emit, ca[r].scatt_cyclosynch_num_ph, ca[r].frame_abs_cnt, ca[r].rebins) == \
            (cnt.num_cyclosynch_ph_emit, cnt.scatt_cyclosynch_num_ph, cnt.frame_abs_cnt, cnt.rebins), r
        got = la[r]
        assert len(got) == len(want) and np.array_equal(got["type"], want["type"]) and np.array_equal(got["weight"], want["weight"])
        for f in ("p0", "r0", "r1", "r2", "s1"):
            scale = np.maximum(np.abs(want["p0"]), 1e-300) if f == "p0" else (np.maximum(np.abs(want[f]), 1e9) if f.startswith("r") else 1.0)
            assert np.all(np.abs(got[f] - want[f]) / scale <= 1e-9), (r, f)


@pytest.mark.parametrize("threads", ["256", "128"])
def test_the_hook_as_a_kernel_between_launches_gives_the_same_lists(hip, oracle, threads, monkeypatch):
    """MCRAT_HIP_CS_HOOK_KERNEL=1 (the hook as cs_replace_pool_kernel between two launches of the loop, the first form of the pool frame) against
    the hook inside the loop kernel: the "2d-rebinning-lists" pool -- a list doubles, a list is parked for rebinning -- comes out the same to the bit."""
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", threads)
    mesh, b_field_calc, max_photons, theta_max, ang_phi, lists = POOLS["2d-rebinning-lists"]
    frame, ph, cfg = synth.config2(n_photons=300, nzc=8, lumi=3e53)
    dens = np.ascontiguousarray(frame["dens"])
    starts = [None if spec is None else _start_list(oracle, ph, 7 * r) for r, spec in enumerate(lists)]
    args = [None if spec is None else dict(seed=spec[0], time_now=0.0, remaining_time=spec[1], r_inj=1e12, ph_weight_suggest=1e40, theta_min=0.0,
                                           theta_max=theta_max, emit_pool=spec[2], scatt_frame_number=200, inj_frame_number=200) for spec in lists]
    runs = {}
    for hook_kernel in ("0", "1"):
        monkeypatch.setenv("MCRAT_HIP_CS_HOOK_KERNEL", hook_kernel)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
        pool.set_hydro(frame)
        pool.set_hydro_extras(dens, None, None, None)
        pool.pool_create(len(lists), 4800)
        for r, before in enumerate(starts):
            if before is not None:
                pool.pool_rank(r, r).set_photons_aos(before.astype(hip.PHOTON_DTYPE))
        sts, cnts = pool.pool_scatter_frames_cyclosynch(args, max_photons, frame["fps"], b_field_calc=b_field_calc, rebin_ang_phi=ang_phi)
        runs[hook_kernel] = (sts, cnts, [None if s is None else pool.pool_rank(r, r).get_photons_aos() for r, s in enumerate(starts)])
        pool.close()
    (sa, ca, la), (sb, cb, lb) = runs["0"], runs["1"]
    grew = rebinned = 0
    for r, spec in enumerate(lists):
        if spec is None:
            continue
        assert sa[r].iterations == sb[r].iterations, r
        assert sa[r].frame_scatt_cnt == sb[r].frame_scatt_cnt, r
        assert (ca[r].num_cyclosynch_ph_emit, ca[r].scatt_cyclosynch_num_ph, ca[r].frame_abs_cnt, ca[r].rebins) == \
            (cb[r].num_cyclosynch_ph_emit, cb[r].scatt_cyclosynch_num_ph, cb[r].frame_abs_cnt, cb[r].rebins), r
        assert len(la[r]) == len(lb[r]), r
        assert la[r].tobytes() == lb[r].tobytes(), r
        grew += len(la[r]) > 600
        rebinned += ca[r].rebins
    assert grew >= 1 and rebinned >= 1                      # the case is the one it is meant to be: a list doubled, a list was parked for rebinning


def test_a_pool_too_small_for_the_doublings_says_so(hip, oracle):
    frame, ph, cfg = synth.config_3d_cartesian(n_photons=300, n=(8, 8, 8))
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
    pool.set_hydro(frame)
    pool.set_hydro_extras(np.ascontiguousarray(frame["dens"]), None, None, None)
    pool.pool_create(1, 1000)                              # 1024 slots: one doubling of 600 does not fit
    pool.pool_rank(0, 0).set_photons_aos(_start_list(oracle, ph, 0).astype(hip.PHOTON_DTYPE))
    with pytest.raises(hip.McratHipError, match="slots per rank|doubl"):
        pool.pool_scatter_frames_cyclosynch([dict(seed=31, time_now=0.0, remaining_time=0.2, r_inj=1e12, ph_weight_suggest=1e40, theta_min=0.0,
                                                  theta_max=0.06, emit_pool=1, scatt_frame_number=200, inj_frame_number=200)], 2000, frame["fps"],
                                            rebin_ang_phi=45.0)
    pool.close()


@pytest.mark.parametrize("shape", ["one-list-context", "pool-views"])
def test_two_frames_with_the_checkpoint_conversion_between_them(hip, oracle, shape):
    """emit -> loop -> rebin/absorb -> saveCheckpoint (every live comptonised photon 'k' becomes an unabsorbed one 'c' in the list,
    mcrat_io.c:896-900) -> printPhotons' PT column -> the next frame, whose absorption counts those 'c' photons (mc_cyclosynch.c:1607) and
    whose rebinning trigger starts from the counter main() carries over (mcrat.c:873): against the oracle doing the same two frames"""
    frame, ph, cfg = synth.config2(n_photons=300, nzc=8, lumi=3e53)
    dens = np.ascontiguousarray(frame["dens"])
    L = oracle.lib()
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], 1)
    H = oracle.OracleHydro(frame)
    max_photons, theta_max = 2000, 0.05
    lists = {"one-list-context": [(31, 0)], "pool-views": [(31, 0), (77, 1)]}[shape]

    def oracle_two_frames(before, seed, stream):
        cs = oracle.CS(1, 0.5, 0.1, dens.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, 200, 200, 0.5, 10.0)
        l = oracle.PhotonList()
        L.orc_list_init(C.byref(l))
        nulls = np.flatnonzero(before["type"] == b"N")
        full = before.copy()
        full[nulls] = before[0]
        assert L.orc_list_set(C.byref(l), full.ctypes.data, len(full)) == 0
        for i in nulls:
            assert L.orc_list_set_null(C.byref(l), int(i)) == 0
        out, t, carry = [], C.c_double(0.0), 0
        for k, rem in enumerate((0.1, 0.1)):
            rng = oracle.Rng()
            L.orc_rng_init(C.byref(rng), seed + k, stream)
            st, cnt = oracle.Stats(), oracle.CSCounts()
            cnt.scatt_cyclosynch_num_ph = carry
            L.orc_scatter_frame_cs(C.byref(c), C.byref(cs), C.byref(l), C.byref(H.c), C.byref(rng), C.byref(t), rem, 1e12, 1e40, max_photons, 0.0, theta_max,
                                   1, 0, C.byref(st), C.byref(cnt))
            assert cnt.error == 0
            converted = L.orc_saveCheckpoint_convert(C.byref(l))
            carry = cnt.scatt_cyclosynch_num_ph
            buf = (C.c_char * (l.list_capacity * oracle.PHOTON_DTYPE.itemsize)).from_address(l.photons)
            out.append((np.frombuffer(buf, dtype=oracle.PHOTON_DTYPE).copy(), st.frame_scatt_cnt, cnt.frame_abs_cnt, cnt.scatt_cyclosynch_num_ph,
                        cnt.num_cyclosynch_ph_emit, converted, t.value))
        L.orc_list_free(C.byref(l))
        return out
    starts = [_start_list(oracle, ph, 11 * r) for r in range(len(lists))]
    wants = [oracle_two_frames(starts[r], seed, stream) for r, (seed, stream) in enumerate(lists)]
    assert wants[0][0][5] > 0 and wants[0][1][2] > 0              # the first frame leaves 'k' photons to convert; the second absorbs

    if shape == "one-list-context":
        e = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
        e.set_hydro(frame)
        e.set_hydro_extras(dens, None, None, None)
        e.set_photons_aos(starts[0].astype(hip.PHOTON_DTYPE))
        views = [e]
    else:
        e = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
        e.set_hydro(frame)
        e.set_hydro_extras(dens, None, None, None)
        e.pool_create(len(lists), 4800)
        views = [e.pool_rank(r, stream) for r, (seed, stream) in enumerate(lists)]
        for r, v in enumerate(views):
            v.set_photons_aos(starts[r].astype(hip.PHOTON_DTYPE))
    t, carry = [0.0] * len(lists), [0] * len(lists)
    for k, rem in enumerate((0.1, 0.1)):
        if shape == "one-list-context":
            tn, st, cnt = e.scatter_frame_cyclosynch(t[0], rem, lists[0][0] + k, 1e12, 1e40, max_photons, 0.0, theta_max, frame["fps"], emit_pool=1,
                                                     scatt_frame_number=200, inj_frame_number=200, scatt_cyclosynch_num_ph=carry[0])
            sts, cnts = [st], [cnt]
        else:
            args = [dict(seed=seed + k, time_now=t[r], remaining_time=rem, r_inj=1e12, ph_weight_suggest=1e40, theta_min=0.0, theta_max=theta_max, emit_pool=1,
                         scatt_frame_number=200, inj_frame_number=200, scatt_cyclosynch_num_ph=carry[r]) for r, (seed, stream) in enumerate(lists)]
            sts, cnts = e.pool_scatter_frames_cyclosynch(args, max_photons, frame["fps"])
        for r, v in enumerate(views):
            want, scatt, absd, carry_w, emit_w, conv_w, t_w = wants[r][k]
            assert (sts[r].frame_scatt_cnt, cnts[r].frame_abs_cnt, cnts[r].scatt_cyclosynch_num_ph, cnts[r].num_cyclosynch_ph_emit) == (scatt, absd, carry_w, emit_w), (k, r)
            assert v.convert_comptonized() == conv_w                                   # what saveCheckpoint does to the list
            v.n = int(v.lib.mcrat_hip_num_photon_slots(v.ctx))
            got = v.get_photons_aos()
            assert len(got) == len(want) and np.array_equal(got["type"], want["type"]), (k, r)
            assert np.array_equal(got["weight"], want["weight"]) and np.array_equal(got["num_scatt"], want["num_scatt"])
            out = v.get_output()                                                        # printPhotons' PT after the checkpoint (mcrat.c:902-907)
            assert np.array_equal(out["type"], want["type"][want["weight"] != 0])
            assert b"k" not in set(out["type"].tolist()) and (k == 0 or b"c" in set(out["type"].tolist()))
            t[r], carry[r] = sts[r].time_now, cnts[r].scatt_cyclosynch_num_ph
            assert t[r] == pytest.approx(t_w, rel=1e-12)
    e.close()
