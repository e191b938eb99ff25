"""The photon storage through the C ABI, where the host's layout rules (mcrat_amd/csrc/photon_plan.hpp; tests/test_photon_plan_cpu.py on the CPU) meet the
device: a list that comes in as columns comes back the same through every read call, at list lengths next to the padding's edges; and while a captured
frame of a rank pool is selected, nothing writes into it."""
import numpy as np
import pytest

from mcrat_amd import synth

pytestmark = pytest.mark.gpu

CAPTURE_TEXT = "a captured frame is selected (mcrat_hip_pool_select_frame(pool, -1) first)"


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _columns(hip, n, seed):
    """a list of n photons as columns, every column its own numbers"""
    rng = np.random.default_rng(seed)
    ph = {f: rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4) for f in hip.F8_COLUMNS}
    ph["p0"] = np.abs(ph["p0"]) + 1e-3
    ph["total_optical_depth"] = np.abs(ph["total_optical_depth"]) + 1e-6
    ph["num_scatt"] = np.floor(np.abs(ph["num_scatt"]))
    ph["s1"][0] = -0.0
    ph["r2"][n - 1] = 5e-324
    ph["weight"][n // 2] = 0.0                                                      # (a photon that does not move)
    ph["type"] = rng.choice(np.array([b"i", b"p", b"c", b"k"], dtype="S1"), n)
    ph["nearest_block_index"] = rng.integers(-1, 1 << 20, n).astype(np.int32)
    ph["recalc_properties"] = rng.integers(0, 2, n).astype(np.int32)
    return ph


def _bit_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [1, 511, 513])
def test_columns_come_back_the_same_through_every_read(hip, n):
    """mcrat_hip_set_photons_soa, then mcrat_hip_get_photons_soa, mcrat_hip_get_photons and mcrat_hip_get_photons_range: the 19 columns, the cell index,
    the type and recalc_properties bit for bit, the records agreeing with the columns -- one slot, one short of the 512-slot padding and one past it"""
    ph = _columns(hip, n, seed=1000 + n)
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    e.set_photons(ph)
    got = e.get_photons()
    names = hip.F8_COLUMNS + ("type", "nearest_block_index", "recalc_properties")
    assert len(hip.F8_COLUMNS) == 19
    for f in names:
        assert _bit_equal(got[f], np.ascontiguousarray(ph[f], dtype=got[f].dtype)), f
    rec = e.get_photons_aos()
    assert len(rec) == n
    for f in names:
        assert _bit_equal(rec[f], got[f].astype(rec[f].dtype)), f
    for first, count in {(0, n), (n - 1, 1), (n // 2, n - n // 2), (max(n - 3, 0), min(3, n))}:
        part = e.get_photons_range(first, count)
        for f in names:
            assert _bit_equal(part[f], rec[f][first:first + count]), (first, count, f)
    e.close()


def _refused(hip, call):
    with pytest.raises(hip.McratHipError) as err:
        call()
    return str(err.value)


def test_nothing_writes_into_a_selected_capture(hip):
    """mcrat_hip_pool_select_frame aims the pool's columns at a captured frame for the read calls.  Every pool entry point that writes photons or loop
    state answers MCRAT_HIP_ESTATE with one text while it is selected, the capture stays bit for bit what it was, and after select_frame(-1) the same
    calls go through.  (mcrat_hip_pool_scatter_frames_cyclosynch can only be refused either way: a pool whose plan was run has the switch off.)"""
    from tests.test_gpu_frame_queue import _pool, _setup
    C = hip.C
    lens = [40, 50]
    frame, cfg, subs, streams = _setup(hip, lens)
    F, R = 2, len(lens)
    fps = frame["fps"]
    q = _pool(hip, frame, cfg, subs, streams, 512)
    assert q.n == R * 512
    q.snapshot_photons()
    seeds = np.array([[77 + 5 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    open_ = np.ones((F, R), dtype=np.int32)
    frame_end = np.array([[(f + 1) / fps for r in range(R)] for f in range(F)])
    run_plan = lambda: q.pool_run_frames(open_, seeds, np.zeros((F, R)), frame_end.copy(), frame_end=frame_end, chain_clock=True, capture=True)
    stats = run_plan()
    assert sum(stats[f][r].frame_scatt_cnt for f in range(F) for r in range(R)) > 0
    recs = [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs]
    o1 = np.ones(R, dtype=np.int32)
    sd1 = np.array([901, 902], dtype=np.uint64)
    t1, rem1 = np.zeros(R), np.full(R, 1.0 / fps)
    _ip, _dp = C.POINTER(C.c_int), C.POINTER(C.c_double)
    begin = lambda: q._check(q.lib.mcrat_hip_pool_begin_frames(q.ctx, o1.ctypes.data_as(_ip), sd1.ctypes.data_as(C.POINTER(C.c_uint64)), t1.ctypes.data_as(_dp),
                                                                rem1.ctypes.data_as(_dp)), "pool_begin_frames")
    inject = dict(r_inj=1e12, ph_weight=1e50, min_photons=1, max_photons=500, spect="b", theta_min=0.0, theta_max=3.0 * np.pi / 180, seed=5)
    cs_list = dict(seed=3, time_now=0.0, remaining_time=1.0 / fps, r_inj=1e12, ph_weight_suggest=1e50, theta_min=0.0, theta_max=0.05)
    writers = [("pool_begin_frames", begin),
               ("run", lambda: q.run(0)),
               ("pool_run_frames", run_plan),
               ("pool_propagate_frames_fast", lambda: q.pool_propagate_frames_fast(o1, sd1, t1, rem1)),
               ("snapshot_photons", q.snapshot_photons),
               ("restore_photons", q.restore_photons),
               ("pool_set_photons", lambda: q.pool_set_photons(list(range(R)), recs)),
               ("pool_inject_photons", lambda: q.pool_inject_photons(fps, [None, inject])),
               ("pool_scatter_frames_cyclosynch", lambda: q.pool_scatter_frames_cyclosynch([cs_list, None], 400, fps))]
    q.pool_select_frame(0)
    before = q.get_photons_range(0, q.n)
    for name, call in writers:
        text = _refused(hip, call)
        assert "call out of order" in text and CAPTURE_TEXT in text, (name, text)          # MCRAT_HIP_ESTATE, the shared text
    after = q.get_photons_range(0, q.n)
    for f in before.dtype.names:                                                    # (field by field: the records' padding bytes are not data)
        assert before[f].tobytes() == after[f].tobytes(), f
    assert before["weight"][:lens[0]].any()                                         # (the capture is not an empty block)
    q.pool_select_frame(-1)
    for name, call in writers[:-1]:
        call()
    assert CAPTURE_TEXT not in _refused(hip, writers[-1][1])                        # the switch is off: refused for that, not for a capture
    q.close()
