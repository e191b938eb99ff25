"""FAST mode (fast_frame_kernel, mcrat_hip_propagate_frame_mode / mcrat_hip_pool_propagate_frames_fast) against its CPU restatement
(oracle/oracle_fast.c), photon for photon: FAST mode is deterministic per photon -- slot i draws the free path of its pass p from the keyed block
{seed, p, i, purpose 8, stream} and its scattering from the event stream {seed, p, i} -- so the bar is the exact loop's: integers and `type` exact,
doubles to 1e-9 (tests.test_gpu_parity._compare), and the frame's counters exact.  tests/test_gpu_fast_mode.py keeps the statistical gates
against the EXACT mode; tests/test_oracle_fast.py pins the restatement itself.

Two decisions of a photon's walk can turn on one rounding of the device's libm: the flight test t < limit and the Klein-Nishina acceptance
test.  The restatement reports the smallest relative margin it saw on each, and every case first asserts, on the CPU, that both exceed 1e-6 -- a
condition on the inputs, met by the choice of the seeds below (a frame of N events comes within about 1/N of a bound; the dense hot case runs a
sixty-fourth of a frame for that reason: 1.3e6 events would come within 1e-6 of a bound whatever the seed, and take 15 s of restatement).
Cell-face ties are dealt with as in the exact mode's parity tests: the same synthetic frames.  No photon is left out of a comparison."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_gpu_instantiations import GEOMS, NAMES, PAIRS, _case, _hot_table
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _lists
from tests.test_oracle_fast import _with_bystanders

pytestmark = pytest.mark.gpu

MARGIN = 1e-6


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


# ------------------------------------------------------------------ the two sides
def _restate(oracle, frame, P, cfg, seed, stream, rem, windows, table=None, slot_base=0):
    """one frame of the restatement on the photons P (in place) -> its counters, after the margin check"""
    H = oracle.OracleHydro(frame)
    okw = dict(hot_table=table) if table is not None else {}
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **okw)
    _, cnt, mg = oracle.fast_frame(c, P, H, seed, stream, rem, windows, slot_base=slot_base)
    assert mg.flight > MARGIN and mg.kn > MARGIN, ("a decision within 1e-6 of turning: choose another seed", seed, mg.flight, mg.kn)
    return cnt


def _photons(oracle, ph):
    return oracle.OraclePhotons(synth.photons_to_aos(ph, oracle.PHOTON_DTYPE))


def _engine(hip, frame, cfg, table=None, **kw):
    if table is not None:
        kw["tau_calculation"] = hip.TAU_TABLE
    e = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], **kw)
    if table is not None:
        e.set_hot_cross_section(table)
    e.set_hydro(frame)
    return e


def _counters(st):
    return dict(iterations=st.iterations, photon_steps=st.photon_steps, frame_scatt_cnt=st.frame_scatt_cnt, kn_rejections=st.kn_rejections,
                num_photons_find_new_element=st.num_photons_find_new_element, not_found=st.not_found)


def _restated_counters(cnt):
    return dict(iterations=cnt.passes, photon_steps=cnt.photon_steps, frame_scatt_cnt=cnt.scatterings, kn_rejections=cnt.kn_rejections,
                num_photons_find_new_element=cnt.relocated, not_found=cnt.not_found)


def _one_list(hip, oracle, frame, ph, cfg, seed, windows, rem=None, stream=0, table=None):
    """one frame of one list on both sides; returns the restatement's counters"""
    rem = 1.0 / frame["fps"] if rem is None else rem
    P = _photons(oracle, ph)
    cnt = _restate(oracle, frame, P, cfg, seed, stream, rem, windows, table)
    e = _engine(hip, frame, cfg, table, rng_stream=stream)
    e.set_photons(ph)
    tn, st = e.propagate_frame_fast(2.0, rem, seed, windows)
    out = e.get_photons()
    e.close()
    assert tn == 2.0 + rem and st.remaining_time == 0.0
    assert _counters(st) == _restated_counters(cnt)
    _compare(out, P.aos)
    return cnt


# ------------------------------------------------------------------ (a) every instantiation of the kernel
# seeds: the first of 100, 101, ... at which the restatement's margins exceed 1e-6 (found on the CPU)
SEEDS_A = {}


@pytest.mark.parametrize("table", [0, 1], ids=["direct", "table"])
@pytest.mark.parametrize("stokes", [0, 1], ids=["stokes-off", "stokes-on"])
@pytest.mark.parametrize("pair", PAIRS, ids=["%s-%s" % (NAMES[d], GEOMS[g]) for d, g in PAIRS])
def test_every_physics_tuple_equals_the_restatement(hip, oracle, pair, stokes, table):
    """DIMENSIONS x GEOMETRY x STOKES x TAU_CALCULATION: 36 builds of the kernel, 501 photons each (the last lane holds half a pair), 8 windows"""
    dims, geom = pair
    frame, ph, cfg = _case(dims, geom, stokes)
    assert len(ph["p0"]) == 501
    seed = SEEDS_A.get((dims, geom, stokes, table), 100)
    cnt = _one_list(hip, oracle, frame, ph, cfg, seed, 8, stream=5, table=_hot_table() if table else None)
    assert cnt.scatterings > 0


# ------------------------------------------------------------------ (b) the clock logic
def _clock_case(which):
    rem = None
    if which == "cfg2":
        frame, ph, cfg = synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=1e54)
    elif which == "cfg3":
        frame, ph, cfg = synth.config3(n_photons=2001, nr=256, nth=128, lumi=1e54)
    elif which == "hot":                                   # T' > 1e7 K: Maxwell-Juettner electrons, Klein-Nishina rejections; 650 scatterings per photon and frame
        frame, ph, cfg = synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=1e54, r_inj=1e11)
        rem = 1.0 / frame["fps"] / 64
    else:                                                  # thin: most photons never scatter, every flight ends on a window boundary
        frame, ph, cfg = synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=3e50)
    ph, null, far, ghost = _with_bystanders(ph)
    return frame, ph, cfg, rem, (null, far, ghost)


SEEDS_B = {("cfg3", 2048): 201}
CLOCK_CASES = [(w, n) for w in ("cfg2", "cfg3") for n in (1, 3, 8, 9, 64, 2048)] + [("hot", 8), ("hot", 64), ("thin", 8), ("thin", 64)]


@pytest.mark.parametrize("which,windows", CLOCK_CASES, ids=["%s-%d" % c for c in CLOCK_CASES])
def test_clocks_and_windows(hip, oracle, which, windows):
    """8 ... 2048 is what the engine clamps a learnt cadence to; an explicit argument goes through as it is, so 1 and 3 run too.  Null slots,
    photons without weight and photons that leave the cells are in every list."""
    frame, ph, cfg, rem, (null, far, ghost) = _clock_case(which)
    cnt = _one_list(hip, oracle, frame, ph, cfg, SEEDS_B.get((which, windows), 200), windows, rem=rem)
    n = len(ph["p0"])
    assert cnt.photon_steps >= windows * (n - null.size - far.size) + null.size
    if which == "hot":
        assert cnt.kn_rejections > 0
    elif which == "thin":
        assert cnt.scatterings < 0.05 * n
        assert cnt.photon_steps == cnt.scatterings + cnt.kn_rejections + windows * (n - null.size - far.size) + null.size + far.size
    else:
        assert cnt.scatterings > n
        if which == "cfg2":
            assert cnt.not_found == far.size                # beyond the mesh, inside the domain (cfg3's mesh fills its domain: they fly out of it)


# ------------------------------------------------------------------ (c) sizes around the launch geometry
SEEDS_C = {}


@pytest.mark.parametrize("n", [1, 2, 511, 512, 513, 1025])
def test_list_sizes_around_the_launch_geometry(hip, oracle, n):
    """a lane takes two photons, a workgroup 512: one lane, one pair, a workgroup less one photon, exactly one, one more, two and a photon"""
    frame, ph, cfg = synth.config2(n_photons=n, nzc=8, stokes=1, lumi=1e54)
    assert len(ph["p0"]) == n
    cnt = _one_list(hip, oracle, frame, ph, cfg, SEEDS_C.get(n, 300), 8)
    assert cnt.photon_steps >= 8 * n and (n < 100 or cnt.scatterings > 0)


# ------------------------------------------------------------------ (d) the lists of a rank pool
SEEDS_D = [400, 420, 440, 460, 480, 500, 520]
POOL_LENS = [1, 63, 65, 300, 1000, 200, 150]           # list 5 stays closed, list 6 is open with no frame time
POOL_STREAMS = [7, 19, 3, 3, 11, 2, 9]
POOL_LUMI = 1e53                                       # some hundred scatterings per thousand photons: learnt cadences inside 8 ... 2048


def _pool_plan(frame):
    dt = 1.0 / frame["fps"]
    rems = [dt, 0.5 * dt, 0.75 * dt, dt, 0.9 * dt, dt, 0.0]
    open_ = [1, 1, 1, 1, 1, 0, 1]
    cadence = {1: 11, 3: 100}                              # two lists with a cadence of their own (mcrat_hip_fast_cadence); the others: 32, a fresh list's
    return rems, open_, cadence


def test_rank_pool_lists_equal_the_restatement_and_their_views_alone(hip, oracle):
    """lists in windows of 1024 slots, each with its seed, stream, frame time and cadence: list-local slot numbers in the keys"""
    frame, ph, cfg = synth.config2(n_photons=sum(POOL_LENS), nzc=8, stokes=1, lumi=POOL_LUMI)
    subs = _lists(ph, POOL_LENS)
    R = len(POOL_LENS)
    rems, open_, cadence = _pool_plan(frame)
    t0 = [1.0 + 0.1 * r for r in range(R)]
    win = [cadence.get(r, 32) for r in range(R)]
    want = []
    for r in range(R):
        P = _photons(oracle, subs[r])
        cnt = _restate(oracle, frame, P, cfg, SEEDS_D[r], POOL_STREAMS[r], rems[r], win[r]) if open_[r] and rems[r] > 0 else None
        want.append((P.aos, cnt))
    pool = _engine(hip, frame, cfg)
    pool.pool_create(R, 1024)
    views = [pool.pool_rank(r, POOL_STREAMS[r]) for r in range(R)]
    for r, v in enumerate(views):
        v.set_photons(subs[r])
        if r in cadence:
            assert v.fast_cadence(cadence[r]) == cadence[r]
        assert v.fast_cadence() == win[r]
    per = pool.pool_propagate_frames_fast(open_, SEEDS_D, t0, rems, 0)
    got = [v.get_photons() for v in views]
    for r in range(R):
        ref, cnt = want[r]
        if cnt is None:                                    # closed, or no frame time: the photons as they were set, byte for byte; the cadence as it was
            for k in got[r]:
                assert np.array_equal(got[r][k], np.asarray(subs[r][k])), (r, k)
            assert views[r].fast_cadence() == win[r]
            if open_[r]:
                assert per[r].frame_scatt_cnt == per[r].photon_steps == per[r].iterations == 0 and per[r].time_now == t0[r]
            continue
        assert _counters(per[r]) == _restated_counters(cnt), r
        assert per[r].time_now == t0[r] + rems[r]
        try:
            _compare(got[r], ref)
        except AssertionError as err:
            raise AssertionError("list %d: %s" % (r, err))
        n = POOL_LENS[r]
        assert views[r].fast_cadence() == min(2048, max(8, int(1000.0 * cnt.scatterings / n + 0.5))), r
    assert sum(w[1].scatterings for w in want if w[1] is not None) > 1000
    # the same lists alone, each through its view: the same bytes
    for r in range(R):
        if want[r][1] is None:
            continue
        views[r].set_photons(subs[r])
        views[r].fast_cadence(win[r])
        tn, st = views[r].propagate_frame_fast(t0[r], rems[r], SEEDS_D[r], 0)
        alone = views[r].get_photons()
        assert _counters(st) == _counters(per[r]) and tn == per[r].time_now
        for k in alone:
            assert np.array_equal(alone[k], got[r][k]), (r, k)
    pool.close()


# ------------------------------------------------------------------ (e) two frames in a row on one context
SEEDS_E = (500, 501)


def test_two_frames_in_a_row_on_one_context(hip, oracle):
    """the second frame starts from the photons as the first left them on the device -- the optical depths the scatterings stored, the flags --
    and runs with another seed"""
    frame, ph, cfg = synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=1e54)
    ph, _, _, _ = _with_bystanders(ph)
    rem = 1.0 / frame["fps"]
    P = _photons(oracle, ph)
    e = _engine(hip, frame, cfg)
    e.set_photons(ph)
    t = 0.0
    for f, seed in enumerate(SEEDS_E):
        cnt = _restate(oracle, frame, P, cfg, seed, 0, rem, 8)
        t, st = e.propagate_frame_fast(t, rem, seed, 8)
        assert _counters(st) == _restated_counters(cnt), f
        assert cnt.scatterings > 2001
        _compare(e.get_photons(), P.aos)
    assert t == 2 * rem
    e.close()


# ------------------------------------------------------------------ (f) a tie in the flight test
def test_a_free_time_equal_to_the_limit_does_not_scatter(hip, oracle):
    """t < limit, not <=.  The one case that is MEANT to sit on a bound (its margin is 0, so no seed can be asked to avoid it): each side is given
    as its frame time the smallest first free time of the list as that side computes it -- the photons' time_to_scatter after a frame too short
    for anything to happen -- so that exactly one photon meets t == limit, on the device with the device's own rounding of the logarithm.  It
    must fly to the end of the frame without scattering (mcrat.c:777: time_to_scatter < remaining_time), like everybody else."""
    frame, ph, cfg = synth.config2(n_photons=64, nzc=8, stokes=1, lumi=1e54)
    seed, n = 600, 64
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    P = _photons(oracle, ph)
    oracle.fast_frame(c, P, H, seed, 0, 1e-30, 1)
    first_cpu = P.aos["time_to_scatter"].copy()
    e = _engine(hip, frame, cfg)
    e.set_photons(ph)
    _, st = e.propagate_frame_fast(0.0, 1e-30, seed, 1)
    first_gpu = e.get_photons()["time_to_scatter"]
    assert st.frame_scatt_cnt == 0 and st.photon_steps == n
    assert np.all(np.abs(first_gpu - first_cpu) <= 1e-9 * first_cpu)
    j = int(np.argmin(first_cpu))
    assert int(np.argmin(first_gpu)) == j and np.sort(first_cpu)[1] > (1 + MARGIN) * first_cpu[j]      # one photon ties, the others are clear of it
    P = _photons(oracle, ph)
    _, cnt, mg = oracle.fast_frame(c, P, H, seed, 0, first_cpu[j], 1)
    assert mg.flight == 0.0                                                       # the tie is there
    assert (cnt.scatterings, cnt.kn_rejections, cnt.photon_steps, cnt.passes) == (0, 0, n, 1)
    e.set_photons(ph)
    _, st = e.propagate_frame_fast(0.0, float(first_gpu[j]), seed, 1)
    assert _counters(st) == _restated_counters(cnt)
    out = e.get_photons()
    e.close()
    assert out["time_to_scatter"][j] == first_gpu[j]
    _compare(out, P.aos)
