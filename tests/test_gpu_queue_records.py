"""The frame queue's host path (mcrat_hip_pool_run_frames): what comes back from a queue launch is one compact record per (frame, list) item
(frame_queue.hpp, FrameRecord) in a buffer that is never cleared, read back with the tickets and frames_done in one copy; the host may read a record
only where frames_done says the kernel wrote it in this call.  None of that may show: every case runs a plan through the queue and through the
same call with MCRAT_HIP_NO_FRAME_QUEUE=1 (one launch per frame, a full LoopState read back per launch) on a second pool, and every field of
every item's mcrat_hip_frame_stats and every photon column must be the same bit for bit -- closed items all zero.  The shapes are the smallest
at which the record path can go wrong: 2-D cylindrical, DIRECT, 256-thread lists with their columns in LDS; ragged lists, a late joiner, a list
that never opens, frames with no time left (the kernel's early return), a pass limit per launch (lists stall, their later items give up and
write nothing, the host relaunches from the records), plans of changing size and openness on ONE pool (a given-up item's place in the buffer
holds an earlier call's record), and the launch forms in turn on one pool (the launcher remembers what it asked the runtime about a kernel).
Through the C ABI."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_parity import FLOAT_FIELDS, INT_FIELDS, _compare
from tests.test_gpu_pool import _lists

pytestmark = pytest.mark.gpu

LENS = [37, 300, 150, 256, 64]
WINDOW = 320
# every member of mcrat_hip_frame_stats but the two that describe the launches themselves (the queue's point is that they differ)
FIELDS = ("iterations", "photon_steps", "frame_scatt_cnt", "num_photons_find_new_element", "not_found", "kn_rejections", "rescans",
          "last_scattered_index", "last_scattered_temp", "last_time_step", "remaining_time", "time_now", "event_kernel_ms", "table_fallbacks",
          "slot_steps")
ORACLE_KEYS = ("iterations", "frame_scatt_cnt", "kn_rejections", "num_photons_find_new_element", "not_found", "last_scattered_index")


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    assert set(FIELDS) | {"step_kernel_ms", "step_kernel_launches"} == {k for k, _ in engine.FrameStats._fields_}
    return engine


@pytest.fixture(scope="module")
def world():
    """one frame and one set of lists for every case (computed once, never changed)"""
    frame, ph, cfg = synth.config2(n_photons=sum(LENS), nzc=8, stokes=1, lumi=1e54)
    return frame, cfg, _lists(ph, LENS), [5 + 3 * r for r in range(len(LENS))]


@pytest.fixture(autouse=True)
def launch_form(monkeypatch):
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", "256")
    for k in ("MCRAT_HIP_NO_LDS_LISTS", "MCRAT_HIP_RANK_LAUNCH_CAP", "MCRAT_HIP_RANK_FUSE", "MCRAT_HIP_NO_FRAME_QUEUE", "MCRAT_HIP_QUEUE_HOST_RECORDS"):
        monkeypatch.delenv(k, raising=False)


def _pool(hip, world, snapshot=False):
    frame, cfg, subs, streams = world
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
    pool.set_hydro(frame)
    pool.pool_create(len(subs), WINDOW)
    for r in range(len(subs)):
        pool.pool_rank(r, streams[r])
    pool.pool_set_photons(list(range(len(subs))), [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs])
    if snapshot:
        pool.snapshot_photons()
    return pool


def _seeds(F, R, base):
    return np.array([[base + 17 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)


def _chained(fps, F, R):
    """plan arrays of a chained clock: every list starts at 0, frame f ends at (f + 1) / fps"""
    end = np.array([[(f + 1) / fps] * R for f in range(F)])
    return dict(time_now=np.zeros((F, R)), remaining_time=end.copy(), frame_end=end, chain_clock=True)


def _restored(fps, F, R):
    return dict(time_now=np.zeros((F, R)), remaining_time=np.full((F, R), 1.0 / fps), restore_each_frame=True)


def _both(monkeypatch, q, ref, open_, seeds, plan, what, launches=1):
    """the plan through the queue on `q` and frame by frame on `ref`; everything equal -> the queue's stats"""
    monkeypatch.delenv("MCRAT_HIP_NO_FRAME_QUEUE", raising=False)
    got = q.pool_run_frames(open_, seeds, **plan)
    monkeypatch.setenv("MCRAT_HIP_NO_FRAME_QUEUE", "1")
    want = ref.pool_run_frames(open_, seeds, **plan)
    monkeypatch.delenv("MCRAT_HIP_NO_FRAME_QUEUE")
    F, R = open_.shape
    if launches == 1:
        assert got[0][0].step_kernel_launches == 1, (what, "the plan did not run as one queue launch", got[0][0].step_kernel_launches)
    elif launches is not None:
        assert got[0][0].step_kernel_launches >= launches, (what, "no list ran into the pass limit", got[0][0].step_kernel_launches)
    for f in range(F):
        for r in range(R):
            for k in FIELDS:
                a, b = getattr(got[f][r], k), getattr(want[f][r], k)
                assert a == b or (a != a and b != b), (what, f, r, k, a, b)
                if not open_[f][r]:
                    assert a == 0, (what, "a closed item's stats are all zero", f, r, k, a)
            if not open_[f][r] and (f, r) != (0, 0):
                assert got[f][r].step_kernel_ms == 0 and got[f][r].step_kernel_launches == 0, (what, f, r)
    for r in range(R):
        a, b = q.views[r].get_photons(), ref.views[r].get_photons()
        for k in FLOAT_FIELDS + INT_FIELDS:
            assert np.array_equal(a[k], b[k], equal_nan=True), (what, "photons of list", r, k)
    return got


def test_ragged_lists_a_late_joiner_and_a_list_that_never_opens(hip, oracle, world, monkeypatch):
    """three chained frames; list 2 joins at frame 1, list 4 never opens (its items' stats are all zero, its photons untouched).  Also against the
    oracle: every open list's frames one after the other on the clock it ended the previous one with"""
    frame, cfg, subs, streams = world
    F, R, fps = 3, len(LENS), frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    open_[0][2] = 0
    open_[:, 4] = 0
    seeds = _seeds(F, R, 1000)
    q, ref = _pool(hip, world), _pool(hip, world)
    got = _both(monkeypatch, q, ref, open_, seeds, _chained(fps, F, R), "late joiner")
    assert sum(got[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0
    untouched = synth.photons_to_aos(subs[4], hip.PHOTON_DTYPE)
    after = q.views[4].get_photons()
    for k in FLOAT_FIELDS + INT_FIELDS:
        assert np.array_equal(after[k], untouched[k], equal_nan=True), ("the list that never opened", k)
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    for r in range(R):
        P = oracle.OraclePhotons(synth.photons_to_aos(subs[r], oracle.PHOTON_DTYPE))
        t = 0.0
        for f in range(F):
            if not open_[f][r]:
                continue
            rst, t, _, _ = oracle.photon_loop(c, P, H, seed=int(seeds[f][r]), time_now=t, remaining_time=(f + 1) / fps - t, stream=streams[r])
            assert tuple(getattr(got[f][r], k) for k in ORACLE_KEYS) == tuple(getattr(rst, k) for k in ORACLE_KEYS), (f, r)
            assert got[f][r].time_now == pytest.approx(t, rel=1e-12), (f, r)
        if open_[:, r].any():
            _compare(q.views[r].get_photons(), P.aos)
    q.close()
    ref.close()


def test_frames_with_no_time_left_report_from_the_early_return(hip, world, monkeypatch):
    """remaining_time == 0 and < 0 in frame 1 of two lists: the item is done before its first pass, and its record is the one the kernel's early
    return writes -- no passes, the clock it was given; the lists go on in frame 2"""
    frame, cfg, subs, streams = world
    F, R, fps = 3, len(LENS), frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    plan = dict(time_now=np.array([[f / fps] * R for f in range(F)]), remaining_time=np.full((F, R), 1.0 / fps))
    plan["remaining_time"][1][1] = 0.0
    plan["remaining_time"][1][3] = -0.25 / fps
    q, ref = _pool(hip, world), _pool(hip, world)
    got = _both(monkeypatch, q, ref, open_, _seeds(F, R, 77), plan, "no time left")
    for r in (1, 3):
        assert got[1][r].iterations == 0 and got[1][r].frame_scatt_cnt == 0 and got[1][r].time_now == 1 / fps
        assert got[1][r].remaining_time == plan["remaining_time"][1][r]
        assert got[0][r].iterations > 0 and got[2][r].iterations > 0
    q.close()
    ref.close()


@pytest.mark.parametrize("mode", ["chain_clock", "restore_each_frame"])
def test_a_pass_limit_relaunches_from_the_records(hip, world, monkeypatch, mode):
    """three passes per list, frame and launch: lists stall, the workgroups of their later items give up (and write no record), and the host
    goes on from frames_done and the stalled frames' records -- launch after launch, to the same photons"""
    frame, cfg, subs, streams = world
    F, R, fps = 3, len(LENS), frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    open_[0][2] = 0
    plan = _chained(fps, F, R) if mode == "chain_clock" else _restored(fps, F, R)
    q, ref = _pool(hip, world, snapshot=True), _pool(hip, world, snapshot=True)
    monkeypatch.setenv("MCRAT_HIP_RANK_LAUNCH_CAP", "3")
    got = _both(monkeypatch, q, ref, open_, _seeds(F, R, 31), plan, mode, launches=2)
    assert max(got[f][r].iterations for f in range(F) for r in range(R)) > 3
    q.close()
    ref.close()


def test_records_of_earlier_calls_are_never_read(hip, world, monkeypatch):
    """one pool, call after call: a plan with every item open fills the records' buffer; a plan of the same size with half the items closed, under
    a pass limit, then meets given-up items whose places hold the first call's records; then a larger and a smaller plan (other offsets into the
    same block).  Every frame starts from the snapshot, so every call has lists that need more than three passes.  Each call equals its
    frame-by-frame run on a pool with the same history"""
    frame, cfg, subs, streams = world
    R, fps = len(LENS), frame["fps"]
    q, ref = _pool(hip, world, snapshot=True), _pool(hip, world, snapshot=True)
    F = 4
    _both(monkeypatch, q, ref, np.ones((F, R), dtype=np.int32), _seeds(F, R, 500), _restored(fps, F, R), "every item open")
    half = np.ones((F, R), dtype=np.int32)
    half[:2, 0::2] = 0                                    # even lists join at frame 2 ...
    half[2:, 1::2] = 0                                    # ... odd ones leave after frame 1
    monkeypatch.setenv("MCRAT_HIP_RANK_LAUNCH_CAP", "3")
    got = _both(monkeypatch, q, ref, half, _seeds(F, R, 600), _restored(fps, F, R), "half closed, pass limit", launches=2)
    assert max(got[f][r].iterations for f in range(F) for r in range(R)) > 3
    for F2, what in ((6, "a larger plan"), (2, "a smaller plan")):
        _both(monkeypatch, q, ref, np.ones((F2, R), dtype=np.int32), _seeds(F2, R, 700 + F2), _restored(fps, F2, R), what + ", pass limit", launches=2)
    monkeypatch.delenv("MCRAT_HIP_RANK_LAUNCH_CAP")
    _both(monkeypatch, q, ref, half, _seeds(F, R, 800), _restored(fps, F, R), "half closed again, no limit")
    q.close()
    ref.close()


def test_the_launch_forms_in_turn_on_one_pool(hip, world, monkeypatch):
    """fused, not fused, fused again: two kernels with their own dynamic-LDS limit and occupancy, asked of the runtime once each -- every call one
    queue launch and the frame-by-frame run's results"""
    frame, cfg, subs, streams = world
    F, R, fps = 3, len(LENS), frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    q, ref = _pool(hip, world, snapshot=True), _pool(hip, world, snapshot=True)
    for k, fuse in enumerate((1, 0, 1, 0)):
        monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
        got = _both(monkeypatch, q, ref, open_, _seeds(F, R, 900 + k), _restored(fps, F, R), "fuse %d, call %d" % (fuse, k))
        assert sum(got[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0
    q.close()
    ref.close()


def test_the_pool_after_a_queue_call(hip, world, monkeypatch):
    """mcrat_hip_rank_stats of every list and a following one-frame mcrat_hip_run on the pool give what they give after the frame-by-frame run:
    the lists' LoopStates on the device are full ones, whatever the host read back"""
    frame, cfg, subs, streams = world
    F, R, fps = 2, len(LENS), frame["fps"]
    open_ = np.ones((F, R), dtype=np.int32)
    open_[1][3] = 0                                       # (its last frame is frame 0)
    q, ref = _pool(hip, world), _pool(hip, world)
    _both(monkeypatch, q, ref, open_, _seeds(F, R, 41), _chained(fps, F, R), "the call before")
    clocks = []
    for r in range(R):
        a, b = q.rank_stats(r), ref.rank_stats(r)
        for k in FIELDS:
            x, y = getattr(a, k), getattr(b, k)
            assert x == y or (x != x and y != y), ("rank_stats", r, k, x, y)
        clocks.append(a.time_now)
    assert clocks[3] < clocks[0]                          # (list 3 stopped a frame earlier)
    out = []
    for pool in (q, ref):
        for r in range(R):
            pool.views[r].begin_frame(4000 + r, clocks[r], (F + 1) / fps - clocks[r])
        out.append(pool.run(0))
    for k in FIELDS:
        x, y = getattr(out[0], k), getattr(out[1], k)
        assert x == y or (x != x and y != y), ("mcrat_hip_run after the call", k, x, y)
    assert out[0].frame_scatt_cnt > 0
    for r in range(R):
        a, b = q.views[r].get_photons(), ref.views[r].get_photons()
        for k in FLOAT_FIELDS + INT_FIELDS:
            assert np.array_equal(a[k], b[k], equal_nan=True), ("after mcrat_hip_run", r, k)
        x, y = q.rank_stats(r), ref.rank_stats(r)
        assert all(getattr(x, k) == getattr(y, k) for k in FIELDS if getattr(x, k) == getattr(x, k)), r
    q.close()
    ref.close()
