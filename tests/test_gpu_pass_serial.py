"""The serial stretch of a rank_loop_kernel pass between phase 1 and the event walk, against the oracle.

A pass sums its counts (re-located slots, slots not found, slots that changed cell) within each wave and adds them to the list's state with one
LDS atomic per wave, in front of the barrier behind the waves' minima; a pass whose slow-path queue is empty has counted everything in phase 1, one
whose queue is not has counts from phase 2 as well.  Where the stretch between phase 1 and the event walk can go wrong: an empty-queue pass next to
one whose queue is not empty; counts summed across waves with idle lanes; the pass's LDS counters against the chunk loop, the end of a frame and
the end of a launch; a list shorter than a wave; TABLE's second round behind its own barrier.  Every case compares as tests/test_gpu_instantiations.py does: integers
(num_photons_find_new_element and the not-found count among them) exact, doubles 1e-9.  Through the C ABI."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _hot_table, _lists
from tests.test_hint_coverage_cpu import hint_coverage

pytestmark = pytest.mark.gpu

STAT_KEYS = ("iterations", "frame_scatt_cnt", "kn_rejections", "num_photons_find_new_element", "not_found", "last_scattered_index")
RAGGED = [1, 63, 65, 300, 1000]
LUMI = 1e51            # between the thin benchmark frame and the dense test frames: about half of a 1000-photon list's slots change cell per pass
LUMI_RAGGED = 5e51     # ... and of a 300-photon list's here; a 63-photon list's nearly all, a 1000-photon list's one in eight
PASSES = 60
ENV = ("MCRAT_HIP_RANK_BLOCK", "MCRAT_HIP_RANK_FUSE", "MCRAT_HIP_NO_LDS_LISTS", "MCRAT_HIP_RANK_LAUNCH_CAP")
# threads per list, fused pass, columns in LDS
FORMS = {"256-fused-resident": (256, 1, 1), "256-unfused-resident": (256, 0, 1), "128": (128, 0, 1), "256-columns-in-hbm": (256, 1, 0)}


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _set_form(monkeypatch, block, fuse, lds, cap=None):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", str(block))
    monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
    if not lds:
        monkeypatch.setenv("MCRAT_HIP_NO_LDS_LISTS", "1")
    if cap is not None:
        monkeypatch.setenv("MCRAT_HIP_RANK_LAUNCH_CAP", str(cap))


def _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, passes, **okw):
    """every list alone through the oracle's loop -> [(records, stats, time_now)]"""
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **okw)
    out = []
    for r, sub in enumerate(subs):
        P = oracle.OraclePhotons(synth.photons_to_aos(sub, oracle.PHOTON_DTYPE))
        rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=seeds[r], time_now=t0, remaining_time=rem, max_iterations=passes, stream=streams[r])
        out.append((P.aos.copy(), rst, rtn))
    return out


def _stats(st, rst):
    """the integer statistics of a list's frame; last_scattered_index only where something has scattered (before the first photonEvent the
    reference's *scattered_ph_index is not set: the oracle's record starts at 0, the engine's at -1)"""
    return tuple(getattr(st, k) for k in STAT_KEYS if k != "last_scattered_index" or rst.frame_scatt_cnt > 0)


def _check_pool(hip, frame, cfg, subs, seeds, streams, t0, rem, passes, want, window, what, setup=None, rtol=1e-9, **kw):
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], **kw)
    if setup:
        setup(pool)
    pool.set_hydro(frame)
    pool.pool_create(len(subs), window)
    for r, sub in enumerate(subs):
        v = pool.pool_rank(r, streams[r])
        v.set_photons(sub)
        v.begin_frame(seeds[r], t0, rem)
    pool.run(passes)
    try:
        for r in range(len(subs)):
            v = pool.pool_rank(r, streams[r])
            st = v.frame_statistics()
            ref, rst, rtn = want[r]
            assert _stats(st, rst) == _stats(rst, rst), (what, r)
            assert st.time_now == pytest.approx(rtn, rel=1e-12), (what, r)
            try:
                _compare(v.get_photons(), ref, rtol=rtol)
            except AssertionError as err:
                raise AssertionError("%s, list %d: %s" % (what, r, err))
    finally:
        pool.close()


def _relocated_share(want, subs):
    """slots re-located per slot-step of the non-forced passes (the forced pass counts none)"""
    return sum(w[1].num_photons_find_new_element for w in want) / max(1, sum((w[1].iterations - 1) * len(s["p0"]) for w, s in zip(want, subs)))


# ---------------------------------------------------------------- ragged lists, four launch forms

@pytest.fixture(scope="module")
def ragged(oracle):
    frame, ph, cfg = synth.config2(n_photons=sum(RAGGED), nzc=8, stokes=0, lumi=LUMI_RAGGED)
    subs = _lists(ph, RAGGED)
    seeds = [911 + 13 * r for r in range(len(RAGGED))]
    streams = [2, 11, 5, 8, 3]
    t0, rem = 0.5, 2.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, PASSES)
    share = [_relocated_share(want[r:r + 1], subs[r:r + 1]) for r in range(len(RAGGED))]
    print("ragged lists: passes %s, events %s, slots re-located per slot and non-forced pass %s"
          % ([w[1].iterations for w in want], [w[1].frame_scatt_cnt for w in want], ["%.2f" % v for v in share]))
    assert all(w[1].frame_scatt_cnt > 0 for w in want[1:]) and want[1][1].iterations > 3
    # RANK_FUSE_DEN: a pass is fused when more than half of the slots changed cell in the one before -- the short lists' passes are, the long list's are not
    assert share[1] > 0.5 > share[4] and 0.2 < share[3] < 0.8
    return frame, cfg, subs, seeds, streams, t0, rem, want


@pytest.mark.parametrize("form", list(FORMS))
def test_ragged_lists_in_one_pool(hip, ragged, monkeypatch, form):
    """lists of 1, 63, 65, 300 and 1000 photons: shorter than a wave, one lane short of one, one over, waves with idle lanes, four slots per thread"""
    frame, cfg, subs, seeds, streams, t0, rem, want = ragged
    _set_form(monkeypatch, *FORMS[form])
    _check_pool(hip, frame, cfg, subs, seeds, streams, t0, rem, PASSES, want, 1024, form)


def test_pass_limit_of_three(hip, ragged, monkeypatch):
    """launches end after three passes of a list and the next launch goes on mid-frame: what a pass leaves in the LDS counters and the list's
    state must not matter to the launch that resumes it"""
    frame, cfg, subs, seeds, streams, t0, rem, want = ragged
    for form in ("256-fused-resident", "256-unfused-resident"):
        _set_form(monkeypatch, *FORMS[form], cap=3)
        _check_pool(hip, frame, cfg, subs, seeds, streams, t0, rem, PASSES, want, 1024, form + ", 3 passes per launch")


def test_ragged_lists_through_the_frame_queue(hip, oracle, monkeypatch):
    """the queue build (persistent workgroups, one (frame, list) item after the other in the same LDS): two chained frames, the 63-photon list
    joins at frame 1"""
    frame, ph, cfg = synth.config2(n_photons=sum(RAGGED), nzc=8, stokes=0, lumi=LUMI_RAGGED)
    subs = _lists(ph, RAGGED)
    R, F, late = len(RAGGED), 2, 1
    streams = [2, 11, 5, 8, 3]
    seeds = np.array([[911 + 13 * r + 1000003 * f for r in range(R)] for f in range(F)], dtype=np.uint64)
    fps = frame["fps"]
    ends = [0.5 / fps, 1.25 / fps]
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    want = []
    for r in range(R):
        P = oracle.OraclePhotons(synth.photons_to_aos(subs[r], oracle.PHOTON_DTYPE))
        row, t = [], 0.0
        for f in range(F):
            if r == late and f == 0:
                row.append(None)
                continue
            rst, t, _, _ = oracle.photon_loop(c, P, H, seed=int(seeds[f][r]), time_now=t, remaining_time=ends[f] - t, stream=streams[r])
            row.append((P.aos.copy(), rst, t))
        want.append(row)
    assert sum(w[1].frame_scatt_cnt for row in want for w in row if w) > 0
    open_ = np.ones((F, R), dtype=np.int32)
    open_[0][late] = 0
    frame_end = np.array([[ends[f]] * R for f in range(F)])
    for fuse in (1, 0):
        _set_form(monkeypatch, 256, fuse, 1)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        pool.pool_create(R, 1024)
        stride = pool.n // R
        for r in range(R):
            pool.pool_rank(r, streams[r]).set_photons(subs[r])
        got = pool.pool_run_frames(open_, seeds, np.zeros((F, R)), frame_end.copy(), frame_end=frame_end, chain_clock=True, capture=True)
        try:
            assert got[0][0].step_kernel_launches == 1, ("fuse %d: the plan did not run as one queue launch" % fuse, got[0][0].step_kernel_launches)
            for f in range(F):
                pool.pool_select_frame(f if f < F - 1 else -1)
                for r in range(R):
                    if want[r][f] is None:
                        assert got[f][r].iterations == 0
                        continue
                    ref, rst, rtn = want[r][f]
                    what = "fuse %d, frame %d, list %d" % (fuse, f, r)
                    assert _stats(got[f][r], rst) == _stats(rst, rst), what
                    assert got[f][r].time_now == pytest.approx(rtn, rel=1e-12), what
                    recs = pool.get_photons_range(r * stride, RAGGED[r]) if f < F - 1 else pool.views[r].get_photons()
                    try:
                        _compare(recs, ref)
                    except AssertionError as err:
                        raise AssertionError("%s: %s" % (what, err))
        finally:
            pool.pool_select_frame(-1)
            pool.close()


# ---------------------------------------------------------------- empty and non-empty queues in one frame

def _straddling_frame(n_photons):
    """cfg2's mesh at nzc = 8 cut so that bucket quadrants straddle cell faces: all coarse cells, and of the fine ones (a quarter of the cells
    or fewer, so that the grid's typical width is the coarse one) those beside the first column and within 4e9 cm of the photons' shell.  The
    radial extent is then 319 fine = 159.5 coarse widths: 159 buckets that drift against the cells, a quadrant in two holds one cell's interior
    or two cells'.  The photons are injected into the cut mesh; those that fly into its gaps are not found, by engine and oracle alike."""
    frame, _, cfg = synth.config2(n_photons=16, nzc=8, stokes=0, lumi=LUMI)
    fine = frame["r0_size"] == frame["r0_size"].min()
    w = float(frame["r0_size"].min())
    keep = ~fine | ((frame["r0"] > w) & (np.abs(frame["r1"] - 1e12) < 4e9))
    sub = synth.select_slab(frame, keep)
    ph = synth.inject_photons(sub, n_photons, 1e12, 0.0, 3.0 * np.pi / 180, 77)
    return sub, ph, cfg


def test_passes_with_and_without_queued_slots(hip, oracle, monkeypatch, tmp_path):
    lens = [300, 1000]
    frame, ph, cfg = _straddling_frame(sum(lens))
    cov = hint_coverage(tmp_path, frame, ph)
    share = 1.0 - cov["hinted"] / cov["points"]
    print("straddling mesh: %d x %d buckets of %.4g x %.4g cm, %.3f of the %d photon positions lie in a quadrant without a hint (%.3f of all quadrants)"
          % (cov["dim"] + cov["width"] + (share, cov["points"], 1.0 - cov["quadrants_hinted"] / cov["quadrants"])))
    assert 0.0 < share < 1.0
    subs = _lists(ph, lens)
    seeds, streams = [31, 47], [6, 9]
    t0, rem = 0.0, 1.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, seeds, streams, t0, rem, PASSES)
    print("   passes %s, events %s, not found %s, %.2f of the slots re-located per non-forced pass"
          % ([w[1].iterations for w in want], [w[1].frame_scatt_cnt for w in want], [w[1].not_found for w in want], _relocated_share(want, subs)))
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    for form in ("256-fused-resident", "256-columns-in-hbm", "256-unfused-resident"):
        _set_form(monkeypatch, *FORMS[form])
        _check_pool(hip, frame, cfg, subs, seeds, streams, t0, rem, PASSES, want, 1024, form)


# ---------------------------------------------------------------- two chunks per pass

def test_a_list_of_two_chunks(hip, oracle, monkeypatch):
    """1100 photons with the columns in HBM: more slots than the slow-path queue holds (4 x 256), so a pass takes phase 1 and phase 2 twice, the
    queue's counter cleared between them, and sums the counts of both chunks once"""
    n = 1100
    frame, ph, cfg = synth.config2(n_photons=n, nzc=8, stokes=0, lumi=LUMI)
    subs = _lists(ph, [n])
    t0, rem = 0.0, 1.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, [5], [4], t0, rem, 40)
    assert want[0][1].frame_scatt_cnt > 0
    for fuse in (1, 0):
        _set_form(monkeypatch, 256, fuse, 0)
        _check_pool(hip, frame, cfg, subs, [5], [4], t0, rem, 40, want, 1100, "fuse %d" % fuse)


# ---------------------------------------------------------------- Stokes on; TABLE with the second round

def test_stokes_on(hip, oracle, monkeypatch):
    lens = [65, 300]
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=1, lumi=LUMI_RAGGED)
    subs = _lists(ph, lens)
    t0, rem = 1.5, 2.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, [21, 22], [1, 2], t0, rem, PASSES)
    assert sum(w[1].frame_scatt_cnt for w in want) > 0
    assert any(np.any(w[0][k] != 0) for w in want for k in ("s1", "s2", "s3"))      # (the scatterings have polarised something)
    for form in ("256-fused-resident", "256-unfused-resident"):
        _set_form(monkeypatch, *FORMS[form])
        _check_pool(hip, frame, cfg, subs, [21, 22], [1, 2], t0, rem, PASSES, want, 512, form)


def test_table_with_deferred_lookups(hip, oracle, monkeypatch):
    """TAU_CALCULATION == TABLE with a table that starts above some photons' energies (built as test_table_lookups_outside_the_table_in_a_rank_pool
    builds its table): their look-ups in phase 2 are deferred to the second round behind its own barrier, a coarse integral of 2560 samples each,
    next to passes in which nothing is deferred.  The table starts at 10^-3.1 m_e c^2, not at 10^-2 as there: with kT <= 1.12e-3 m_e c^2 in this
    frame an electron of the integral has gamma <= 1 + 12 theta = 1.0134 and beta <= 0.162, so a deferred photon's energy in the electron's frame
    stays below 10^-3.1 x 1.0134 x 1.162 = 9.4e-4 < 1e-3: every sample takes the Klein-Nishina formula's linear branch, none the branch above its
    1e-3 seam whose cancellation of terms of 1e6 is why that test compares at 1e-6 (measured here with the table from 10^-2: 1.49e-9 in
    total_optical_depth).  So the 1e-9 gate applies to the deferred values too."""
    lens = [70, 130]
    tab, grid, calls, passes = _hot_table(), (-3.1, 6.0, -4.0, 4.0), 2560, 40
    frame, ph, cfg = synth.config2(n_photons=sum(lens), nzc=8, stokes=1, lumi=1e54)
    subs = _lists(ph, lens)
    t0, rem = 1.5, 1.0 / frame["fps"]
    want = _want(oracle, frame, cfg, subs, [500, 501], [3, 4], t0, rem, passes, hot_table=tab, grid=grid, fallback_calls=calls)
    assert float(frame["temp"].max()) * 1.380649e-16 / 8.1871e-7 <= 1.12e-3
    assert all(w[1].table_fallbacks > 0 for w in want) and sum(w[1].frame_scatt_cnt for w in want) > 0
    assert sum(w[1].table_fallbacks for w in want) < 20          # (a few deferred look-ups: most passes have none)

    def setup(pool):
        pool.set_hot_cross_section(tab, grid)
        pool.table_fallback_calls(calls)
    _set_form(monkeypatch, 256, 0, 1)
    _check_pool(hip, frame, cfg, subs, [500, 501], [3, 4], t0, rem, passes, want, 256, "table", setup=setup, tau_calculation=hip.TAU_TABLE)
