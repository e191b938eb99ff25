"""The fused pass over lists of every trip count, and the in-kernel restore of the frame queue, against the oracle.

Two things the other files' shapes do not reach (their lists are 64-300 slots, or the comparison is with another launch form only):

- Trip counts.  A pass of rank_loop_kernel (kernels.hip) takes a list in chunks of 4 x threads slots (RANK_QCAP); within a chunk a thread of the fused
  form takes one slot pair per trip (RANK_NS_FUSED = 2), so a trip of a 256-thread list covers 512 slots and a chunk 1024.  With 256 threads:
      255, 256, 257, 511 slots   one trip (odd last slot: 255, 257, 511; idle threads in the trip: all four)
      513, 1016, 1023 slots      two trips (513: thread 0 alone in the second; 1023: odd last slot; 1016: four threads without a second pair)
      1025, 1026, 1087 slots     three trips, the third being the SECOND CHUNK (c0 = 1024: the barriers between chunks, the reset of the slow-path
                                 queue), with one pair of which one slot (1025), one whole pair (1026) and 32 pairs, the last odd (1087)
  (the 256-thread builds with their columns in LDS, queue builds included, take lists of up to 1088 slots: launch_rank_loop).  With 512 threads a
  trip covers 1024 slots and a chunk 2048: one trip up to 1023 slots, two above.  In the queue form (four slots per thread and trip) a 256-thread
  list makes one trip per chunk.  Every such list through the fused builds -- with the frame queue and without, columns in LDS and in HBM/L2, 512
  threads too -- and through the builds without the fused pass must give the oracle's photons and counters: integers exact, doubles 1e-9.
- A queue launch of a restoring plan takes every fresh (frame, list) item from the snapshot inside the kernel: the columns a list keeps in LDS go
  straight there, the others to the live lists (restore_list_columns_lds).  A restored plan in which one list has no time left in a frame (the
  early return keeps the full copy), one list runs into the launch's pass limit and is resumed by the next launch from its live columns, and a
  frame is captured after its restore: each list after each frame against the oracle and against the plan run one launch per frame.

A queue launch that cannot be made falls back to one launch per frame without an error, so the launch counts are asserted.  Through the C ABI."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _lists
from tests.test_gpu_queue_instantiations import STAT_KEYS, _oracle_frames

pytestmark = pytest.mark.gpu

LENS = [255, 256, 257, 511, 513, 1016, 1023, 1025, 1026, 1087]
WINDOW = 1088                                             # the longest list the 256-thread builds keep in LDS (launch_rank_loop)
PASSES = 24
TUPLES = [(synth.TWO, synth.CYLINDRICAL, 0), (synth.THREE, synth.POLAR, 1), (synth.TWO, synth.SPHERICAL, 1)]
IDS = ["2d-cylindrical", "3d-polar-stokes", "2d-spherical-stokes"]


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _case(dims, geom, stokes, n):
    if dims == synth.TWO and geom == synth.CYLINDRICAL:
        frame, ph, cfg = synth.config2(n_photons=n, nzc=8, stokes=stokes, lumi=1e54)
    elif dims == synth.TWO:
        frame, ph, cfg = synth.config3(n_photons=n, nr=256, nth=128, stokes=stokes, lumi=1e54)
    else:
        frame, ph, cfg = synth.config_3d(geom, n_photons=n, stokes=stokes)
    return frame, ph, dict(cfg, stokes=int(stokes))


def _fuses(geom):
    """MCRAT_HIP_RANK_FUSE values that select a build of their own (kernels.hip, launch_rank_loop: no fused pass in spherical geometry)"""
    return (0, 1) if geom != synth.SPHERICAL else (0,)


def _check(st, recs, ref, rst, rtn, what):
    assert tuple(getattr(st, k) for k in STAT_KEYS) == tuple(getattr(rst, k) for k in STAT_KEYS), what
    assert st.time_now == pytest.approx(rtn, rel=1e-12), what
    try:
        _compare(recs, ref)
    except AssertionError as err:
        raise AssertionError("%s: %s" % (what, err))


@pytest.mark.parametrize("tup", TUPLES, ids=IDS)
def test_lists_of_every_trip_count_without_the_queue(hip, oracle, monkeypatch, tup):
    dims, geom, stokes = tup
    frame, ph, cfg = _case(dims, geom, stokes, sum(LENS))
    subs = _lists(ph, LENS)
    R = len(LENS)
    seeds = [977 + 13 * r for r in range(R)]
    streams = [3 + 2 * r for r in range(R)]
    t0, rem = 0.5, 1.0 / frame["fps"]
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    want = []
    for r in range(R):
        P = oracle.OraclePhotons(synth.photons_to_aos(subs[r], oracle.PHOTON_DTYPE))
        rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=seeds[r], time_now=t0, remaining_time=rem, max_iterations=PASSES, stream=streams[r])
        want.append((P.aos.copy(), rst, rtn))
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    forms = [(256, fuse, lds) for fuse in _fuses(geom) for lds in (1, 0)] + [(512, fuse, 1) for fuse in _fuses(geom)]
    for block, fuse, lds in forms:
        monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", str(block))
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
        if lds:
            monkeypatch.delenv("MCRAT_HIP_NO_LDS_LISTS", raising=False)
        else:
            monkeypatch.setenv("MCRAT_HIP_NO_LDS_LISTS", "1")
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
        pool.set_hydro(frame)
        pool.pool_create(R, WINDOW)
        for r in range(R):
            v = pool.pool_rank(r, streams[r])
            v.set_photons(subs[r])
            v.begin_frame(seeds[r], t0, rem)
        pool.run(PASSES)
        for r in range(R):
            v = pool.pool_rank(r, streams[r])
            ref, rst, rtn = want[r]
            _check(v.frame_statistics(), v.get_photons(), ref, rst, rtn, "threads %d, fuse %d, LDS %d, list of %d" % (block, fuse, lds, LENS[r]))
        pool.close()


@pytest.mark.parametrize("tup", TUPLES, ids=IDS)
def test_lists_of_every_trip_count_through_the_queue(hip, oracle, monkeypatch, tup):
    """two chained frames, the first captured, in ONE queue launch (as tests/test_gpu_queue_instantiations.py, with these lists)"""
    dims, geom, stokes = tup
    frame, ph, cfg = _case(dims, geom, stokes, sum(LENS))
    subs = _lists(ph, LENS)
    R, F = len(LENS), 2
    seeds = np.array([[515 + 29 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    streams = [3 + 2 * r for r in range(R)]
    t0 = 0.5
    rem, frame_end, want = _oracle_frames(oracle, frame, cfg, subs, [[int(s) for s in row] for row in seeds], streams, t0, {})
    assert sum(w[f][1].frame_scatt_cnt for w in want for f in range(F)) > 0
    open_ = np.ones((F, R), dtype=np.int32)
    ends = np.array([[frame_end[f]] * R for f in range(F)])
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "256")
    monkeypatch.delenv("MCRAT_HIP_NO_LDS_LISTS", raising=False)
    monkeypatch.delenv("MCRAT_HIP_RANK_LAUNCH_CAP", raising=False)
    for fuse in _fuses(geom):
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        pool.pool_create(R, WINDOW)
        stride = pool.n // R                              # (the pool rounds its windows up)
        for r in range(R):
            pool.pool_rank(r, streams[r]).set_photons(subs[r])
        got = pool.pool_run_frames(open_, seeds, np.full((F, R), t0), np.full((F, R), rem), frame_end=ends, chain_clock=True, capture=True)
        assert got[0][0].step_kernel_launches == 1, ("fuse %d: the plan did not run as one queue launch" % fuse, got[0][0].step_kernel_launches)
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            for r in range(R):
                ref, rst, rtn = want[r][f]
                recs = pool.get_photons_range(r * stride, LENS[r]) if f < F - 1 else pool.views[r].get_photons()
                _check(got[f][r], recs, ref, rst, rtn, "fuse %d, frame %d, list of %d" % (fuse, f, LENS[r]))
        pool.close()


R_LENS = [255, 513, 1016, 1023, 400, 1087]
SLOW, IDLE0, IDLE1 = 2, 1, 4                              # the list with the long frames; the lists with no time left in frame 0 / in frame 1
K = 12                                                    # list 0's events in a frame of the restored plan


@pytest.mark.parametrize("fuse", [0, 1], ids=["queue-form", "fused"])
@pytest.mark.parametrize("tup", TUPLES[:2], ids=IDS[:2])
def test_a_restored_plan_with_an_idle_list_a_stalled_list_and_a_capture(hip, oracle, monkeypatch, tup, fuse):
    """restore_each_frame, two frames, frame 0 captured; a frame lasts until halfway between list 0's K-th and (K+1)-th event.  List IDLE0 has
    remaining_time = 0 in frame 0 and IDLE1 in frame 1 (restored by the early return's full copy: the capture / the live list is the snapshot); list
    SLOW has frames three times as long as the others', and the pass limit per launch is put between the others' longest frame and SLOW's shortest
    (both taken from the oracle's pass counts), so that exactly SLOW stalls in each of its frames and is resumed by a later launch from its live
    columns.  With and without that limit; every list after every frame against the oracle, and bit for bit against the plan run one launch per
    frame.  The launch counts: without the limit one; with it, SLOW's frame 1 starts in the launch that ends its frame 0, so the queue needs one
    launch less than the frame-by-frame path, which takes each frame's launches one after the other."""
    dims, geom, stokes = tup
    F, R = 2, len(R_LENS)
    frame, ph, cfg = _case(dims, geom, stokes, sum(R_LENS))
    subs = _lists(ph, R_LENS)
    streams = [5 + 3 * r for r in range(R)]
    seeds = np.array([[2000 + 17 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    ends = []
    for k in (K, K + 1):
        P = oracle.OraclePhotons(synth.photons_to_aos(subs[0], oracle.PHOTON_DTYPE))
        rst, rtn, rrem, _ = oracle.photon_loop(c, P, H, seed=int(seeds[0][0]), time_now=0.0, remaining_time=100.0 / frame["fps"], max_iterations=k,
                                               stream=streams[0])
        assert rst.iterations == k and rrem > 0
        ends.append(rtn)
    assert ends[1] > ends[0]
    rem = np.full((F, R), 0.5 * (ends[0] + ends[1]))
    rem[:, SLOW] *= 3
    rem[0][IDLE0] = 0.0
    rem[1][IDLE1] = 0.0
    open_ = np.ones((F, R), dtype=np.int32)
    want = {}
    for f in range(F):
        for r in range(R):
            if rem[f][r] <= 0:
                continue
            P = oracle.OraclePhotons(synth.photons_to_aos(subs[r], oracle.PHOTON_DTYPE))
            rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=int(seeds[f][r]), time_now=0.0, remaining_time=float(rem[f][r]), stream=streams[r])
            want[f, r] = (P.aos.copy(), rst, rtn)
    cap = max(w[1].iterations for (f, r), w in want.items() if r != SLOW) + 1
    assert min(want[f, SLOW][1].iterations for f in range(F)) > cap, "the long frames must need more passes than the others"
    assert sum(w[1].frame_scatt_cnt for w in want.values()) > 0
    per_frame = [-(-want[f, SLOW][1].iterations // cap) for f in range(F)]              # launches SLOW's frame f needs under the limit (>= 2 each)
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "256")
    monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
    monkeypatch.delenv("MCRAT_HIP_NO_LDS_LISTS", raising=False)

    def run(one_by_one, limit):
        for k, v in (("MCRAT_HIP_NO_FRAME_QUEUE", "1" if one_by_one else None), ("MCRAT_HIP_RANK_LAUNCH_CAP", str(limit) if limit else None)):
            if v is None:
                monkeypatch.delenv(k, raising=False)
            else:
                monkeypatch.setenv(k, v)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        pool.pool_create(R, WINDOW)
        for r in range(R):
            pool.pool_rank(r, streams[r])
        pool.pool_set_photons(list(range(R)), [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs])
        pool.snapshot_photons()
        stride = pool.n // R                              # (the pool rounds its windows up)
        snap = pool.get_photons_range(0, R * stride)
        got = pool.pool_run_frames(open_, seeds, np.zeros((F, R)), rem, restore_each_frame=True, capture=True)
        recs = []
        for f in range(F):
            pool.pool_select_frame(f if f < F - 1 else -1)
            recs.append(pool.get_photons_range(0, R * stride))
        pool.pool_select_frame(-1)
        pool.close()
        monkeypatch.delenv("MCRAT_HIP_NO_FRAME_QUEUE", raising=False)
        monkeypatch.delenv("MCRAT_HIP_RANK_LAUNCH_CAP", raising=False)
        return got, recs, snap, stride

    ref_got, ref_recs, _, _ = run(True, None)
    assert ref_got[0][0].step_kernel_launches >= F
    for limit in (None, cap):
        got, recs, snap, stride = run(False, limit)
        launches = got[0][0].step_kernel_launches
        print("limit %s: %d launches; SLOW's frames need %s passes" % (limit, launches, [want[f, SLOW][1].iterations for f in range(F)]))
        if limit is None:
            assert launches == 1, ("the plan did not run as one queue launch", launches)
        else:
            # the plan's launch stalls in frame 0; the launch that ends frame 0 starts frame 1, which stalls in turn: at least three, and one less
            # than a launch per `cap` passes of each frame one after the other (which is what the plan costs frame by frame)
            assert 3 <= launches <= sum(per_frame) - 1, (launches, per_frame)
        for f in range(F):
            for r in range(R):
                what = "limit %s, frame %d, list %d" % (limit, f, r)
                mine = recs[f][r * stride:r * stride + R_LENS[r]]
                theirs = ref_recs[f][r * stride:r * stride + R_LENS[r]]
                for name in mine.dtype.names:
                    assert np.array_equal(mine[name], theirs[name], equal_nan=mine[name].dtype.kind == "f"), (what, name)
                if rem[f][r] <= 0:
                    assert got[f][r].iterations == 0, what
                    before = snap[r * stride:r * stride + R_LENS[r]]
                    for name in mine.dtype.names:
                        assert np.array_equal(mine[name], before[name], equal_nan=mine[name].dtype.kind == "f"), (what, name, "not the snapshot")
                    continue
                ref, rst, rtn = want[f, r]
                _check(got[f][r], mine, ref, rst, rtn, what)
