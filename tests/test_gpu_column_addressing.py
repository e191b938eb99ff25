"""rank_loop_kernel's column addressing against the oracle: a global column as a scalar base plus the slot's 32-bit byte offset, an LDS column at a
compile-time pitch (the launch form's slot limit: mcrat_amd/csrc/photon_cols.hpp, rank_form_plan.hpp).

Where addressing can go wrong: a list that does not start at slot 0 (the byte offset counts from the block's first slot, the LDS index from the
list's); lists shorter than a wave, one lane short of one, one over, several trips per thread; the last list's last slot being the block's last; the
same slot reached through LDS in one launch form and through global memory in another; the restore of the frame queue, which fills the LDS copy
without the accessor; lists that occupy less than the LDS pitch and exactly the pitch.  Every launch form runs the same lists through the same frame:
each list must equal the oracle's trajectory as tests/test_gpu_pass_serial.py compares it (integers exact, doubles 1e-9), and the forms must agree
with each other bit for bit.

A pool's windows are multiples of 512 slots (mcrat_hip_pool_create), so in a pool every list starts at a multiple of 16 and a 1000-photon list ends 24
slots short of the block's end; the lists that start at slots that are no multiple of 16, the last of them ending at the block's last slot (slot
n_pad - 1 = 1023 of a block of 1024), are the virtual ranks of one context (test_virtual_ranks_at_odd_slots).  Those run every launch form but the
frame queue: a plan of frames is a rank pool's (mcrat_hip_pool_run_frames returns MCRAT_HIP_ESTATE for any other context), so the queue and its
restore inside the kernel only ever see lists at multiples of 512 slots; they run on the pools here.  Through the C ABI."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_parity import _compare
from tests.test_gpu_pass_serial import _set_form, _stats, _want
from tests.test_gpu_pool import _hot_table, _lists

pytestmark = pytest.mark.gpu

RAGGED = [1, 63, 65, 300, 1000]
LUMI_RAGGED = 5e51       # as tests/test_gpu_pass_serial.py: short lists' passes are fused, the long list's are not
STREAMS = [2, 11, 5, 8, 3]
# threads per list, fused pass, columns in LDS
FORMS = {"256-fused-resident": (256, 1, 1), "256-unfused-resident": (256, 0, 1), "256-columns-in-hbm": (256, 1, 0), "128": (128, 0, 1)}


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _same_bits(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), (what, k)


def _run_views(hip, frame, cfg, subs, seeds, streams, t0, rem, window, setup=None, passes=0, **kw):
    """one launch per frame: every list begun through its view -> [(records, FrameStats)]"""
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], **kw)
    try:
        if setup:
            setup(pool)
        pool.set_hydro(frame)
        pool.pool_create(len(subs), window)
        views = [pool.pool_rank(r, streams[r]) for r in range(len(subs))]
        for r, v in enumerate(views):
            v.set_photons(subs[r])
            v.begin_frame(seeds[r], t0, rem)
        pool.run(passes)
        return [(v.get_photons(), v.frame_statistics()) for v in views]
    finally:
        pool.close()


def _run_queue(hip, frame, cfg, subs, seeds, streams, rem, window):
    """the frame queue with the restore inside the kernel: two frames, each from the snapshot; frame 1 is the one compared (its seeds are `seeds`)"""
    R, F = len(subs), 2
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
    try:
        pool.set_hydro(frame)
        pool.pool_create(R, window)
        views = [pool.pool_rank(r, streams[r]) for r in range(R)]
        pool.pool_set_photons(list(range(R)), [synth.photons_to_aos(s, hip.PHOTON_DTYPE) for s in subs])
        pool.snapshot_photons()
        plan_seeds = np.array([[s + 77 for s in seeds], seeds], dtype=np.uint64)
        got = pool.pool_run_frames(np.ones((F, R), dtype=np.int32), plan_seeds, np.zeros((F, R)), np.full((F, R), rem), restore_each_frame=True)
        assert got[0][0].step_kernel_launches == 1, ("the plan did not run as one queue launch", got[0][0].step_kernel_launches)
        return [(views[r].get_photons(), got[F - 1][r]) for r in range(R)]
    finally:
        pool.close()


def _against_oracle(got, want, what, rtol=1e-9):
    for r, ((recs, st), (ref, rst, rtn)) in enumerate(zip(got, want)):
        assert _stats(st, rst) == _stats(rst, rst), (what, r)
        assert st.time_now == pytest.approx(rtn, rel=1e-12), (what, r)
        try:
            _compare(recs, ref, rtol=rtol)
        except AssertionError as err:
            raise AssertionError("%s, list %d: %s" % (what, r, err))


def _forms_agree(runs):
    first = next(iter(runs))
    for what, got in runs.items():
        for r, ((recs, st), (recs0, st0)) in enumerate(zip(got, runs[first])):
            _same_bits(recs, recs0, "%s against %s, list %d" % (what, first, r))
            assert (st.iterations, st.frame_scatt_cnt, st.time_now) == (st0.iterations, st0.frame_scatt_cnt, st0.time_now), (what, r)


# ---------------------------------------------------------------- ragged lists, every launch form

@pytest.fixture(scope="module")
def ragged(oracle):
    frame, ph, cfg = synth.config2(n_photons=sum(RAGGED), nzc=8, stokes=0, lumi=LUMI_RAGGED)
    subs = _lists(ph, RAGGED)
    seeds = [911 + 13 * r for r in range(len(RAGGED))]
    t0, rem = 0.0, 2.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, seeds, STREAMS, t0, rem, 0)
    print("ragged lists: passes %s, events %s" % ([w[1].iterations for w in want], [w[1].frame_scatt_cnt for w in want]))
    assert all(w[1].frame_scatt_cnt > 0 for w in want[1:]) and want[1][1].iterations > 3
    return frame, cfg, subs, seeds, t0, rem, want


def test_ragged_lists_in_every_launch_form(hip, ragged, monkeypatch):
    """lists of 1, 63, 65, 300 and 1000 photons in one pool: 256 threads fused and unfused with the columns in LDS, the same with the columns in
    HBM/L2 (MCRAT_HIP_NO_LDS_LISTS=1), 128 threads (r and -1/tau in LDS, the rest global), and the frame queue with its restore"""
    frame, cfg, subs, seeds, t0, rem, want = ragged
    runs = {}
    for form, (block, fuse, lds) in FORMS.items():
        _set_form(monkeypatch, block, fuse, lds)
        runs[form] = _run_views(hip, frame, cfg, subs, seeds, STREAMS, t0, rem, 1024)
    for fuse in (1, 0):
        _set_form(monkeypatch, 256, fuse, 1)
        runs["queue-restore-fuse-%d" % fuse] = _run_queue(hip, frame, cfg, subs, seeds, STREAMS, rem, 1024)
    for what, got in runs.items():
        _against_oracle(got, want, what)
    _forms_agree(runs)


@pytest.mark.parametrize("longest", [1000, 1072, 1073, 1088])
def test_lists_below_and_at_the_lds_pitch(hip, oracle, monkeypatch, longest):
    """256-thread lists keep their columns in LDS 1088 slots apart: lists that occupy 1008 of them, 1072, and -- 1073 and 1088 photons -- all 1088,
    the last slot of the last LDS column included; each next to a 65-photon list, and equal to the same lists with the columns in HBM/L2"""
    lens = [longest, 65]
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=0, lumi=LUMI_RAGGED)
    subs = _lists(ph, lens)
    seeds, streams = [41, 42], [7, 1]
    t0, rem = 0.0, 0.25 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, 0)
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    runs = {}
    for form in ("256-fused-resident", "256-unfused-resident", "256-columns-in-hbm"):
        _set_form(monkeypatch, *FORMS[form])
        runs[form] = _run_views(hip, frame, cfg, subs, seeds, streams, t0, rem, 1088)
    _set_form(monkeypatch, 256, 1, 1)
    runs["queue-restore"] = _run_queue(hip, frame, cfg, subs, seeds, streams, rem, 1088)
    for what, got in runs.items():
        _against_oracle(got, want, what)
    _forms_agree(runs)


# ---------------------------------------------------------------- lists that start at slots that are no multiple of 16

def test_virtual_ranks_at_odd_slots(hip, oracle, monkeypatch):
    """one context cut into lists of 301 slots: they start at slots 301, 602 and 903, and the last one (121 photons) ends at slot 1023, the last slot of
    the block (the layout pads to a multiple of 512 slots: n = n_pad = 1024, every column's last element is a list's)"""
    per, tail = 301, 121
    n = 3 * per + tail
    assert n % 512 == 0 and all((r * per) % 16 for r in (1, 2, 3))
    frame, ph, cfg = synth.config2(n_photons=n, nzc=8, stokes=0, lumi=LUMI_RAGGED)
    subs = _lists(ph, [per, per, per, tail])
    seed, first_stream = 31, 5
    t0, rem = 0.0, 2.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, [seed] * 4, [first_stream + r for r in range(4)], t0, rem, 0)
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    outs = {}
    for form, (block, fuse, lds) in FORMS.items():
        _set_form(monkeypatch, block, fuse, lds)
        e = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], rng_stream=first_stream, virtual_rank_photons=per)
        try:
            e.set_hydro(frame)
            e.set_photons(ph)
            assert e.num_virtual_ranks() == 4
            e.begin_frame(seed, t0, rem)
            e.run(0)
            out = e.get_photons()
            for r, (ref, rst, rtn) in enumerate(want):
                lo, hi = r * per, min((r + 1) * per, n)
                st = e.rank_stats(r)
                assert (st.iterations, st.frame_scatt_cnt, st.kn_rejections, st.num_photons_find_new_element) == \
                       (rst.iterations, rst.frame_scatt_cnt, rst.kn_rejections, rst.num_photons_find_new_element), (form, r)
                assert st.time_now == pytest.approx(rtn, rel=1e-12), (form, r)
                try:
                    _compare({k: v[lo:hi] for k, v in out.items()}, ref)
                except AssertionError as err:
                    raise AssertionError("%s, list %d: %s" % (form, r, err))
            outs[form] = out
        finally:
            e.close()
    first = next(iter(outs))
    for form, out in outs.items():
        for k, v in out.items():
            assert np.asarray(v).tobytes() == np.asarray(outs[first][k]).tobytes(), (form, k)


# ---------------------------------------------------------------- Stokes on; TABLE

def test_stokes_on(hip, oracle, monkeypatch):
    lens = [65, 300]
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=1, lumi=LUMI_RAGGED)
    subs = _lists(ph, lens)
    seeds, streams = [21, 22], [1, 2]
    t0, rem = 0.0, 2.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, 0)
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    assert any(np.any(w[0][k] != 0) for w in want for k in ("s1", "s2", "s3"))      # (the scatterings have polarised something)
    runs = {}
    for form, (block, fuse, lds) in FORMS.items():
        _set_form(monkeypatch, block, fuse, lds)
        runs[form] = _run_views(hip, frame, cfg, subs, seeds, streams, t0, rem, 512)
    _set_form(monkeypatch, 256, 1, 1)
    runs["queue-restore"] = _run_queue(hip, frame, cfg, subs, seeds, streams, rem, 512)
    for what, got in runs.items():
        _against_oracle(got, want, what)
    _forms_agree(runs)


def test_table(hip, oracle, monkeypatch):
    """TAU_CALCULATION == TABLE (no fused build): 256 threads with the columns in LDS and in HBM/L2, and 128 threads; 40 passes of a dense frame"""
    lens = [70, 130]
    tab = _hot_table()
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=1, lumi=1e54)
    subs = _lists(ph, lens)
    seeds, streams = [500, 501], [3, 4]
    t0, rem, passes = 1.5, 1.0 / frame["fps"], 40
    want = _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, passes, hot_table=tab)
    assert sum(w[1].frame_scatt_cnt for w in want) > 0

    def setup(pool):
        pool.set_hot_cross_section(tab)
    runs = {}
    for form in ("256-unfused-resident", "256-columns-in-hbm", "128"):
        _set_form(monkeypatch, *FORMS[form])
        runs[form] = _run_views(hip, frame, cfg, subs, seeds, streams, t0, rem, 256, setup=setup, passes=passes, tau_calculation=hip.TAU_TABLE)
    for what, got in runs.items():
        _against_oracle(got, want, what)
    _forms_agree(runs)
