"""Tapes for the lists of a rank pool (mcrat_hip_pool_set_rng_tapes): the tape build of rank_loop_kernel against the oracle.

MCRaT is run as many MPI ranks, each with its own generator (mcrat.c:99-103,701); a maintainer who records several ranks replays them as the lists
of one pool, each list reading its own tape in MCRaT's call order -- per pass one gsl_rng_uniform_pos per located slot in ascending slot order
(mclib.c:646-675), then photonEvent's draws.  Every list is held against oracle.photon_loop(..., tape=that list's tape): counters and the tape
position exact, time_now 1e-12, photons through tests.test_gpu_parity._compare (integers exact, doubles 1e-9).  Lists without a tape keep their keyed
streams bit for bit.  Through the C ABI."""
import ctypes as C

import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_instantiations import GEOMS, LENS, NAMES, PAIRS, _case
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _hot_table, _lists
from tests.test_gpu_tape import _tape

pytestmark = pytest.mark.gpu

K = 24                      # list 0's events in the first frame
STAT_KEYS = ("iterations", "frame_scatt_cnt", "kn_rejections", "num_photons_find_new_element", "last_scattered_index")
ALL_KEYS = STAT_KEYS + ("photon_steps", "slot_steps", "not_found", "rescans", "last_scattered_temp", "last_time_step", "remaining_time", "time_now")


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _pool_tape(n, seed, zero_every=0, passes=4 * K):
    """enough uniforms for `passes` passes of a list of n photons; zeros inside the first pass's free-path draws (gsl_rng_uniform_pos skips them),
    and further ones every `zero_every` entries"""
    t = _tape(passes * (n + 300) + 20000, seed, zero_every)
    t[3] = 0.0
    t[10:13] = 0.0
    return t


def _oracle(oracle, frame, cfg, sub, tape, t0, rem, tape_pos=0, max_iterations=0, okw=None):
    """-> (photons after, stats, time_now, tape position) of one list through the oracle on its tape"""
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **(okw or {}))
    P = oracle.OraclePhotons(synth.photons_to_aos(sub, oracle.PHOTON_DTYPE))
    rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=0, time_now=t0, remaining_time=rem, max_iterations=max_iterations, tape=tape, tape_pos=tape_pos)
    return P.aos.copy(), rst, rtn, oracle.photon_loop.tape_pos


def _frame_length(oracle, frame, cfg, sub, tape, t0, okw):
    """a frame that ends halfway between list 0's K-th and (K+1)-th events: no event of it lies within rounding of the frame's end"""
    probe = 100.0 / frame["fps"]
    ends = []
    for k in (K, K + 1):
        _, rst, rtn, _ = _oracle(oracle, frame, cfg, sub, tape, t0, probe, max_iterations=k, okw=okw)
        assert rst.iterations == k
        ends.append(rtn)
    assert ends[1] > ends[0]
    return 0.5 * (ends[0] + ends[1]) - t0


def _check(what, st, pos, ran_out, got, want):
    ref, rst, rtn, rpos = want
    assert not ran_out, what
    assert tuple(getattr(st, k) for k in STAT_KEYS) == tuple(getattr(rst, k) for k in STAT_KEYS), what
    assert pos == rpos, what
    assert st.time_now == pytest.approx(rtn, rel=1e-12), what
    try:
        _compare(got, ref)
    except AssertionError as err:
        raise AssertionError("%s: %s" % (what, err))


def _same(a, b, what):
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), (what, k)


def _same_stats(a, b, what):
    for k in ALL_KEYS:
        x, y = getattr(a, k), getattr(b, k)
        assert x == y or (x != x and y != y), (what, k, x, y)


def _begin_frames(pool, open_, seeds, time_now, remaining):
    R = pool.n_pool_ranks
    o = (C.c_int * R)(*[int(x) for x in open_])
    sd = (C.c_uint64 * R)(*[int(x) for x in seeds])
    t = (C.c_double * R)(*[float(x) for x in time_now])
    rem = (C.c_double * R)(*[float(x) for x in remaining])
    pool._check(pool.lib.mcrat_hip_pool_begin_frames(pool.ctx, o, sd, t, rem), "pool_begin_frames")


@pytest.mark.parametrize("table", [0, 1], ids=["direct", "table"])
@pytest.mark.parametrize("stokes", [0, 1], ids=["stokes-off", "stokes-on"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % (NAMES[d], GEOMS[g]) for d, g in PAIRS])
def test_every_tape_build_equals_the_oracle(hip, oracle, pair, stokes, table):
    """each physics tuple's tape build: ragged lists run to the end of a frame, beside a list that sits the frame out and an empty window; in 2-D a
    second frame reads on from every list's position"""
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, stokes)
    subs = _lists(ph, LENS)
    # windows: 0, 1, 4 open lists; 2 a list that sits the frame out (with a tape); 3 no list at all
    lists = {0: subs[0], 1: subs[1], 2: subs[2], 4: subs[2]}
    R = 5
    tapes = [_pool_tape(len(lists[r]["p0"]), 100 + r) if r in lists else None for r in range(R)]
    kw, okw = {}, {}
    if table:
        kw, okw = dict(tau_calculation=hip.TAU_TABLE), dict(hot_table=_hot_table())
    t0 = 1.5
    rem = _frame_length(oracle, frame, cfg, lists[0], tapes[0], t0, okw)
    opened = (0, 1, 4)
    want = {r: _oracle(oracle, frame, cfg, lists[r], tapes[r], t0, rem, okw=okw) for r in opened}
    assert sum(want[r][1].frame_scatt_cnt for r in opened) > 0

    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], **kw)
    if table:
        pool.set_hot_cross_section(okw["hot_table"])
    pool.set_hydro(frame)
    pool.pool_create(R, 512)
    views = {r: pool.pool_rank(r, 7 + r) for r in lists}
    for r, sub in lists.items():
        views[r].set_photons(sub)
    pool.pool_set_rng_tapes(tapes)
    for r in opened:
        views[r].begin_frame(4242 + r, t0, rem)
    st = pool.run(0)
    if table:
        assert st.table_fallbacks == 0
    pos, ran_out = pool.pool_rng_tape_positions()
    assert pos[2] == 0 and pos[3] == 0 and not ran_out[2]
    for r in opened:
        _check("list %d" % r, views[r].frame_statistics(), pos[r], ran_out[r], views[r].get_photons(), want[r])
        assert views[r].frame_statistics().remaining_time <= 0
    _compare(views[2].get_photons(), synth.photons_to_aos(lists[2], oracle.PHOTON_DTYPE))     # (sat the frame out: as it was set)

    if dims == synth.TWO:                                  # the next frame reads on from each list's position
        H = oracle.OracleHydro(frame)
        c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **okw)
        for r in opened:
            views[r].begin_frame(9 + r, want[r][2], rem)
        pool.run(0)
        pos2, ran_out2 = pool.pool_rng_tape_positions()
        for r in opened:
            P = oracle.OraclePhotons(want[r][0].copy())
            rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=0, time_now=want[r][2], remaining_time=rem, tape=tapes[r], tape_pos=want[r][3])
            assert pos2[r] > pos[r]
            _check("frame 2, list %d" % r, views[r].frame_statistics(), pos2[r], ran_out2[r], views[r].get_photons(),
                   (P.aos, rst, rtn, oracle.photon_loop.tape_pos))
    pool.close()


ONE_LIST_CASES = {
    "cfg1-cartesian": (lambda: synth.config1(n_photons=700, n0=32, n1=32), 1000),
    "cfg2-cylindrical-stokes": (lambda: synth.config2(n_photons=900, nzc=8, stokes=1, lumi=1e54), 1000),
    "cfg3-spherical-stokes": (lambda: synth.config3(n_photons=800, nr=256, nth=128, lumi=1e54), 0),
    # T >= 1e7 K: the keyed build samples the electron with the wave-parallel sampler, the tape build with the serial one (physics.hpp)
    "cfg2-hot-maxwell-juttner": (lambda: synth.config2(n_photons=600, nzc=8, stokes=0, lumi=1e54, r_inj=1e11), 500),
}


@pytest.mark.parametrize("case", list(ONE_LIST_CASES))
def test_a_taped_list_equals_the_one_list_tape_path(hip, case):
    """every list of a taped pool against a context of its own holding that list and its tape (mcrat_hip_set_rng_tape: step_kernel,
    tape_draw_kernel, event_kernel) -- two different routes through the same recorded streams"""
    make, zero_every = ONE_LIST_CASES[case]
    frame, ph, cfg = make()
    n = len(ph["p0"])
    lens = [n // 3, n // 2, n - n // 3 - n // 2]
    subs = _lists(ph, lens)
    tapes = [_pool_tape(m, 31 + r, zero_every) for r, m in enumerate(lens)]
    rem, passes = 1.0 / frame["fps"], 60
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(len(lens), max(lens))
    views = [pool.pool_rank(r, r) for r in range(len(lens))]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
        v.begin_frame(5 + r, 0.25, rem)
    pool.pool_set_rng_tapes(tapes)
    pool.run(passes)
    pos, ran_out = pool.pool_rng_tape_positions()
    scattered = 0
    for r, v in enumerate(views):
        one = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], iterations_per_sync=16)
        one.set_hydro(frame)
        one.set_photons(subs[r])
        one.set_rng_tape(tapes[r])
        one.begin_frame(1, 0.25, rem)
        ost = one.run(passes)
        opos, oran = one.rng_tape_position()
        st = v.frame_statistics()
        what = "%s, list %d" % (case, r)
        assert not ran_out[r] and not oran, what
        assert tuple(getattr(st, k) for k in STAT_KEYS) == tuple(getattr(ost, k) for k in STAT_KEYS), what
        assert pos[r] == opos, what
        assert st.time_now == pytest.approx(ost.time_now, rel=1e-12), what
        got, ref = v.get_photons(), one.get_photons()
        _compare(got, {k: np.asarray(ref[k]) for k in ref})
        scattered += st.frame_scatt_cnt
        one.close()
    assert scattered > 0
    pool.close()


def _mixed_pool(hip, frame, cfg, subs, tapes, seeds, passes, rem):
    """a pool of len(subs) lists, tapes[r] None: keyed -> (pool, per list (stats, photons))"""
    R = len(subs)
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(R, 512)
    views = [pool.pool_rank(r, 3 + 2 * r) for r in range(R)]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
    if tapes is not None:
        pool.pool_set_rng_tapes(tapes)
    _begin_frames(pool, [1] * R, seeds, [0.5] * R, [rem] * R)
    pool.run(passes)
    return pool, views, [(v.frame_statistics(), v.get_photons()) for v in views]


def test_a_mixed_pool_keeps_its_keyed_lists_and_ignores_the_taped_lists_seeds(hip):
    frame, ph, cfg = synth.config2(n_photons=1600, nzc=8, stokes=1, lumi=1e54)
    lens = [400, 350, 450, 400]
    subs = _lists(ph, lens)
    rem, passes = 1.0 / frame["fps"], 80
    tapes = [_pool_tape(lens[0], 70), None, _pool_tape(lens[2], 72), None]
    seeds_a, seeds_b = [11, 12, 13, 14], [901, 902, 903, 904]
    pool_a, _, a = _mixed_pool(hip, frame, cfg, subs, tapes, seeds_a, passes, rem)
    pos_a, _ = pool_a.pool_rng_tape_positions()
    assert pos_a[0] > 0 and pos_a[2] > 0 and pos_a[1] == 0 and pos_a[3] == 0
    keyed_pool, _, k = _mixed_pool(hip, frame, cfg, subs, None, seeds_a, passes, rem)
    for r in (1, 3):                                       # the keyed lists of the taped pool: as in a pool without tapes, bit for bit
        _same_stats(a[r][0], k[r][0], "keyed list %d" % r)
        _same(a[r][1], k[r][1], "keyed list %d" % r)
    pool_b, _, b = _mixed_pool(hip, frame, cfg, subs, tapes, seeds_b, passes, rem)
    for r in (0, 2):                                       # the taped lists: their tape decides, not their seed
        _same_stats(a[r][0], b[r][0], "taped list %d" % r)
        _same(a[r][1], b[r][1], "taped list %d" % r)
    assert not np.array_equal(a[1][1]["p0"], b[1][1]["p0"])
    assert not np.array_equal(a[0][1]["p0"], k[0][1]["p0"])
    # clearing the tapes gives the keyed results back, bit for bit
    pool_a.pool_set_rng_tapes([None] * len(subs))
    views = [pool_a.pool_rank(r, 3 + 2 * r) for r in range(len(subs))]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
    _begin_frames(pool_a, [1] * len(subs), seeds_a, [0.5] * len(subs), [rem] * len(subs))
    pool_a.run(passes)
    for r, v in enumerate(views):
        _same_stats(v.frame_statistics(), k[r][0], "cleared, list %d" % r)
        _same(v.get_photons(), k[r][1], "cleared, list %d" % r)
    with pytest.raises(hip.McratHipError):
        pool_a.pool_rng_tape_positions()                   # (no tapes any more)
    for p in (pool_a, keyed_pool, pool_b):
        p.close()


@pytest.mark.parametrize("shape", ["many-short-lists-128", "few-long-lists-512"])
def test_list_shapes_the_keyed_mode_sends_elsewhere_run_the_tape_build(hip, oracle, monkeypatch, shape):
    """many short lists (the keyed mode's 128-thread lists) and a few long ones (512 threads, several chunks of a pass): the tape build all the same,
    whatever MCRAT_HIP_RANK_* ask for"""
    if shape.startswith("many"):
        lens = [40 + (13 * r) % 37 for r in range(600)]
        monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "128")
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", "0")
    else:
        lens = [2100, 1700]
        monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "512")
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", "1")
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=0, lumi=1e54)
    subs = _lists(ph, lens)
    R = len(lens)
    rem, passes = 1.0 / frame["fps"], 40
    tapes = [_pool_tape(m, 500 + r, passes=2 * passes) for r, m in enumerate(lens)]
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(R, max(lens))
    for r in range(R):
        pool.pool_rank(r, r)
    pool.pool_set_photons(list(range(R)), [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs])
    pool.pool_set_rng_tapes(tapes)
    _begin_frames(pool, [1] * R, [77 + r for r in range(R)], [0.0] * R, [rem] * R)
    pool.run(passes)
    pos, ran_out = pool.pool_rng_tape_positions()
    check = range(R) if R < 16 else sorted(np.random.default_rng(7).choice(R, 12, replace=False).tolist())
    for r in check:
        v = pool.pool_rank(r, r)
        want = _oracle(oracle, frame, cfg, subs[r], tapes[r], 0.0, rem, max_iterations=passes)
        _check("%s, list %d" % (shape, r), v.frame_statistics(), pos[r], ran_out[r], v.get_photons(), want)
    assert not ran_out.any()
    pool.close()


def test_a_frame_plan_with_tapes_equals_frame_by_frame(hip, oracle):
    frame, ph, cfg = synth.config2(n_photons=900, nzc=8, stokes=0, lumi=1e54)
    lens = [300, 250, 350]
    subs = _lists(ph, lens)
    R, F = len(lens), 2
    tapes = [_pool_tape(m, 600 + r) for r, m in enumerate(lens)]
    rem = _frame_length(oracle, frame, cfg, subs[0], tapes[0], 0.0, {})
    seeds = np.array([[3 + r + 100 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    t_first = np.array([[0.0] * R, [rem] * R])

    def make():
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        pool.pool_create(R, 512)
        for r in range(R):
            pool.pool_rank(r, r).set_photons(subs[r])
        pool.pool_set_rng_tapes(tapes)
        return pool

    ref = make()
    ref_stats, ref_photons, ref_pos = [], [], []
    for f in range(F):
        _begin_frames(ref, [1] * R, seeds[f], t_first[f], [rem] * R)
        ref.run(0)
        ref_stats.append([ref.pool_rank(r, r).frame_statistics() for r in range(R)])
        ref_photons.append([ref.pool_rank(r, r).get_photons() for r in range(R)])
        pos, ran_out = ref.pool_rng_tape_positions()
        assert not ran_out.any()
        ref_pos.append(pos)
    assert (ref_pos[1] > ref_pos[0]).all()

    pool = make()
    stride = pool.n // R
    got = pool.pool_run_frames(np.ones((F, R), dtype=np.int32), seeds, t_first, np.full((F, R), rem), capture=True)
    assert got[0][0].step_kernel_launches >= F                # (one launch per frame: the tape build has no queue form)
    pos, ran_out = pool.pool_rng_tape_positions()
    assert not ran_out.any() and np.array_equal(pos, ref_pos[1])
    for f in range(F):
        pool.pool_select_frame(f if f < F - 1 else -1)
        for r in range(R):
            what = "frame %d, list %d" % (f, r)
            _same_stats(got[f][r], ref_stats[f][r], what)
            recs = pool.get_photons_range(r * stride, lens[r])
            want = ref_photons[f][r]
            for k in ("p0", "p1", "r0", "r1", "r2", "num_scatt", "weight"):
                assert np.array_equal(recs[k], want[k]), (what, k)
    pool.pool_select_frame(-1)
    assert sum(got[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0
    pool.close()
    ref.close()


def test_a_short_tape_runs_out_for_its_own_list_only(hip, oracle):
    frame, ph, cfg = synth.config2(n_photons=900, nzc=8, stokes=0, lumi=1e54)
    lens = [300, 300, 300]
    subs = _lists(ph, lens)
    rem, passes = 1.0 / frame["fps"], 30
    tapes = [_pool_tape(300, 40), _pool_tape(300, 41)[:450], _pool_tape(300, 42)]    # list 1: one pass and a half
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(3, 512)
    views = [pool.pool_rank(r, r) for r in range(3)]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
        v.begin_frame(1 + r, 0.0, rem)
    pool.pool_set_rng_tapes(tapes)
    pool.run(passes)
    pos, ran_out = pool.pool_rng_tape_positions()
    assert list(ran_out) == [False, True, False]
    assert pos[1] >= len(tapes[1])
    for r in (0, 2):
        want = _oracle(oracle, frame, cfg, subs[r], tapes[r], 0.0, rem, max_iterations=passes)
        _check("list %d" % r, views[r].frame_statistics(), pos[r], ran_out[r], views[r].get_photons(), want)
    pool.close()


def test_tapes_are_refused_where_they_have_no_meaning(hip):
    frame, ph, cfg = synth.config2(n_photons=600, nzc=8, stokes=0, lumi=1e54)
    subs = _lists(ph, [300, 300])
    good = _pool_tape(300, 1)
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    pool.set_hydro(frame)
    pool.pool_create(2, 512)
    views = [pool.pool_rank(r, r) for r in range(2)]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
    for bad in (1.0, -0.1, np.nan):                        # gsl_rng_uniform returns [0, 1)
        t = good.copy()
        t[5] = bad
        with pytest.raises(hip.McratHipError, match="outside"):
            pool.pool_set_rng_tapes([good, t])
    with pytest.raises(hip.McratHipError):
        pool.pool_rng_tape_positions()                     # (nothing was set)
    with pytest.raises(hip.McratHipError, match="rank pool"):
        views[0].pool_set_rng_tapes([good])                # a view
    with pytest.raises(hip.McratHipError):
        views[0].pool_rng_tape_positions()
    single = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    with pytest.raises(hip.McratHipError, match="rank pool"):
        single.pool_set_rng_tapes([good])                  # a context without lists
    single.close()
    pool.pool_set_rng_tapes([good, None])
    with pytest.raises(hip.McratHipError, match="tapes"):
        pool.pool_propagate_frames_fast([1, 1], [1, 2], [0.0, 0.0], [1.0 / frame["fps"]] * 2)
    views[0].begin_frame(1, 0.0, 1.0 / frame["fps"])
    with pytest.raises(hip.McratHipError, match="tapes"):
        views[0].run(3)                                    # a view alone would draw from its keyed streams
    pool.close()
    cs = hip.Engine(cfg["dimensions"], cfg["geometry"], 1, cyclosynchrotron=1)
    cs.pool_create(2, 1000)
    with pytest.raises(hip.McratHipError, match="cyclo-synchrotron"):
        cs.pool_set_rng_tapes([good, None])
    cs.close()
