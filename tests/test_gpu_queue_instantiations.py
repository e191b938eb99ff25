"""EVERY queue build of rank_loop_kernel (QUEUE = true: mcrat_hip_pool_run_frames, the frame queue) against the oracle.

The queue builds exist for 256-thread lists with their columns in LDS only, with the fused pass wherever the non-queue builds have one (DIRECT, not
spherical): 48 instantiations, every one at 256 VGPRs with scalar registers spilled to vector lanes and scratch (profiles/r04_kernel_resources.txt) --
the class of build in which the compiler's spill path once wrote a wrong Stokes V.  tests/test_gpu_instantiations.py holds the non-queue builds to
the oracle; here each physics tuple's queue builds run a two-frame plan (the clock carried over, every frame but the last captured) and must give
the oracle's photons and counters after each frame: integers exact, doubles 1e-9.  A queue launch that cannot be made falls back to one launch
per frame without an error, so every form also asserts that ONE launch ran.

The frames end halfway between two of list 0's events (its K-th and (K+1)-th), so that no event of it lies within rounding of a frame's end.
Through the C ABI."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_instantiations import GEOMS, LENS, NAMES, PAIRS, _case
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _hot_table, _lists

pytestmark = pytest.mark.gpu

K = 20                      # list 0's events per frame
WINDOW = 512
STAT_KEYS = ("iterations", "frame_scatt_cnt", "kn_rejections", "num_photons_find_new_element", "not_found", "last_scattered_index")


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _queue_forms(table, geom):
    """MCRAT_HIP_RANK_FUSE values that select a queue build of their own (kernels.hip, launch_rank_loop)"""
    return (0, 1) if (not table and geom != synth.SPHERICAL) else (0,)


def _oracle_frames(oracle, frame, cfg, subs, seeds, streams, t0, okw):
    """two chained frames per list on one OraclePhotons -> (frame length, [per list: (records, stats, time_now) after frame 0, after frame 1])"""
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **okw)
    aos = [synth.photons_to_aos(s, oracle.PHOTON_DTYPE) for s in subs]
    probe = 100.0 / frame["fps"]
    ends = []
    for k in (K, K + 1):
        P = oracle.OraclePhotons(aos[0].copy())
        rst, rtn, rrem, _ = oracle.photon_loop(c, P, H, seed=seeds[0][0], time_now=t0, remaining_time=probe, max_iterations=k, stream=streams[0])
        assert rst.iterations == k and rrem > 0
        ends.append(rtn)
    assert ends[1] > ends[0]
    rem = 0.5 * (ends[0] + ends[1]) - t0
    frame_end = (t0 + rem, t0 + 2 * rem)
    want = []
    for r in range(len(subs)):
        P = oracle.OraclePhotons(aos[r].copy())
        rst0, rtn0, _, _ = oracle.photon_loop(c, P, H, seed=seeds[0][r], time_now=t0, remaining_time=rem, stream=streams[r])
        after0 = P.aos.copy()
        rst1, rtn1, _, _ = oracle.photon_loop(c, P, H, seed=seeds[1][r], time_now=rtn0, remaining_time=frame_end[1] - rtn0, stream=streams[r])
        want.append(((after0, rst0, rtn0), (P.aos.copy(), rst1, rtn1)))
    assert want[0][0][1].iterations == K + 1              # the K events, then the step to the frame's end
    return rem, frame_end, want


@pytest.mark.parametrize("table", [0, 1], ids=["direct", "table"])
@pytest.mark.parametrize("stokes", [0, 1], ids=["stokes-off", "stokes-on"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % (NAMES[d], GEOMS[g]) for d, g in PAIRS])
def test_every_queue_build_of_a_physics_tuple_equals_the_oracle(hip, oracle, monkeypatch, pair, stokes, table):
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, stokes)
    subs = _lists(ph, LENS)
    R, F = len(LENS), 2
    seeds = np.array([[4242 + 31 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    streams = [7, 19, 3]
    t0 = 1.5
    kw, okw = {}, {}
    if table:
        kw, okw = dict(tau_calculation=hip.TAU_TABLE), dict(hot_table=_hot_table())
    rem, frame_end, want = _oracle_frames(oracle, frame, cfg, subs, [[int(s) for s in row] for row in seeds], streams, t0, okw)
    assert sum(w[f][1].frame_scatt_cnt for w in want for f in range(F)) > 0
    open_ = np.ones((F, R), dtype=np.int32)
    t_first = np.full((F, R), t0)
    rem_first = np.full((F, R), rem)
    ends = np.array([[frame_end[f]] * R for f in range(F)])
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "256")
    monkeypatch.delenv("MCRAT_HIP_NO_LDS_LISTS", raising=False)
    monkeypatch.delenv("MCRAT_HIP_RANK_LAUNCH_CAP", raising=False)
    # (MCRAT_HIP_NO_FRAME_QUEUE is left as it is: a suite run with the queue switched off fails here instead of passing without it)
    for fuse in _queue_forms(table, geom):
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True, **kw)
        if table:
            pool.set_hot_cross_section(okw["hot_table"])
        pool.set_hydro(frame)
        pool.pool_create(R, WINDOW)
        stride = pool.n // R                              # (the pool rounds its windows up)
        for r in range(R):
            pool.pool_rank(r, streams[r]).set_photons(subs[r])
        got = pool.pool_run_frames(open_, seeds, t_first, rem_first, frame_end=ends, chain_clock=True, capture=True)
        assert got[0][0].step_kernel_launches == 1, ("fuse %d: the plan did not run as one queue launch" % fuse, got[0][0].step_kernel_launches)
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            for r in range(R):
                ref, rst, rtn = want[r][f]
                what = "fuse %d, frame %d, list %d" % (fuse, f, r)
                st = got[f][r]
                assert tuple(getattr(st, k) for k in STAT_KEYS) == tuple(getattr(rst, k) for k in STAT_KEYS), what
                assert st.time_now == pytest.approx(rtn, rel=1e-12), what
                recs = pool.get_photons_range(r * stride, LENS[r]) if f < F - 1 else pool.views[r].get_photons()
                try:
                    _compare(recs, ref)
                except AssertionError as err:
                    raise AssertionError("%s: %s" % (what, err))
        pool.close()


def test_the_benchmark_plan_equals_the_oracle(hip, oracle, monkeypatch):
    """bench.py's plan shape and build: 2-D cylindrical, Stokes off, DIRECT, the fused queue build, every frame from the snapshot with its own
    seeds -- with many more (frame, list) items than the device holds at once, so that every persistent workgroup takes several.  Every list and
    frame against the same plan run one launch per frame; a seeded sample of lists against the oracle, every frame"""
    lens = [48 + (7 * r) % 33 for r in range(700)]
    F, R, window = 3, len(lens), 96
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=0, lumi=1e54)
    subs = _lists(ph, lens)
    streams = [5 + 3 * r for r in range(R)]
    seeds = np.array([[1000 + 17 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    rem = 1.0 / frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "256")
    monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", "1")
    monkeypatch.delenv("MCRAT_HIP_NO_LDS_LISTS", raising=False)
    monkeypatch.delenv("MCRAT_HIP_RANK_LAUNCH_CAP", raising=False)
    def run(one_by_one):
        if one_by_one:
            monkeypatch.setenv("MCRAT_HIP_NO_FRAME_QUEUE", "1")
        else:
            monkeypatch.delenv("MCRAT_HIP_NO_FRAME_QUEUE", raising=False)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        pool.pool_create(R, window)
        for r in range(R):
            pool.pool_rank(r, streams[r])
        pool.pool_set_photons(list(range(R)), [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs])
        pool.snapshot_photons()
        stride = pool.n // R                              # (the pool rounds its windows up)
        got = pool.pool_run_frames(open_, seeds, np.zeros((F, R)), np.full((F, R), rem), restore_each_frame=True, capture=True)
        recs = []
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            recs.append(pool.get_photons_range(0, R * stride))
        pool.pool_select_frame(-1)
        pool.close()
        return got, recs, stride

    got, recs, stride = run(False)
    assert got[0][0].step_kernel_launches == 1, ("the plan did not run as one queue launch", got[0][0].step_kernel_launches)
    ref, ref_recs, _ = run(True)
    slots = np.concatenate([np.arange(r * stride, r * stride + lens[r]) for r in range(R)])
    assert ref[0][0].step_kernel_launches >= F
    keys = ("iterations", "photon_steps", "frame_scatt_cnt", "num_photons_find_new_element", "not_found", "kn_rejections", "rescans",
            "last_scattered_index", "last_scattered_temp", "last_time_step", "remaining_time", "time_now")
    for f in range(F):
        for r in range(R):
            for k in keys:
                a, b = getattr(got[f][r], k), getattr(ref[f][r], k)
                assert a == b or (a != a and b != b), (f, r, k, a, b)
        a, b = recs[f][slots], ref_recs[f][slots]
        for name in a.dtype.names:
            assert np.array_equal(a[name], b[name], equal_nan=a[name].dtype.kind == "f"), (f, name)
    assert sum(got[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0

    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    for r in sorted(np.random.default_rng(2026).choice(R, 16, replace=False).tolist()):
        for f in range(F):
            P = oracle.OraclePhotons(synth.photons_to_aos(subs[r], oracle.PHOTON_DTYPE))
            rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=int(seeds[f][r]), time_now=0.0, remaining_time=rem, stream=streams[r])
            st = got[f][r]
            what = "frame %d, list %d" % (f, r)
            assert tuple(getattr(st, k) for k in STAT_KEYS) == tuple(getattr(rst, k) for k in STAT_KEYS), what
            assert st.time_now == pytest.approx(rtn, rel=1e-12), what
            try:
                _compare(recs[f][r * stride:r * stride + lens[r]], P.aos)
            except AssertionError as err:
                raise AssertionError("%s: %s" % (what, err))
