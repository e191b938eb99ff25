"""The cell lookup through the covered-octant table (GridDev::cov_back; physics.hpp find_in_bucket, kernels.hip relocate_lockstep), on the device.

The table of a frame is built by grid_finish_kernel with the rule of hydro_plan.hpp (octant_covered) and must equal the host build's
(MCRAT_HIP_HOST_GRID=1).  A position whose octant is covered takes its cell from the 4-B entry and the cell's values from the cell's own record
instead of the hinted bucket-list entry: every decision and every value are the ones the path through the bucket records gives, so a run is
compared with the oracle (integers exact, doubles 1e-9, as tests/test_gpu_parity.py's _compare does) AND byte for byte with the same run under
MCRAT_HIP_NO_COVERED=1.  Lists of 1, 63, 65, 300 and 1000 photons (shorter than a wave, one lane short, one over, idle lanes, four slots per
thread), 24 passes, through the launch forms of the rank pool, the frame queue and the list mode's step_kernel; meshes: config2(nzc=8) at
lumi = 1e54, the same mesh cut so that covered and uncovered quadrants lie side by side (and gaps), 2.5-D (the third velocity component comes
from the cell's record) and 3-D polar with Stokes parameters (eight octants per bucket); the first two also as thin as the benchmark's frame."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests.test_covered_octants_cpu import cut_mesh, driver, frame_columns, run_mesh  # noqa: F401  (driver: the fixture that compiles the CPU driver)
from tests.test_gpu_parity import _compare
from tests.test_gpu_pool import _lists

pytestmark = pytest.mark.gpu

STAT_KEYS = ("iterations", "frame_scatt_cnt", "kn_rejections", "num_photons_find_new_element", "not_found", "last_scattered_index")
RAGGED = [1, 63, 65, 300, 1000]
PASSES = 24
SEEDS = [911 + 13 * r for r in range(len(RAGGED))]
STREAMS = [2, 11, 5, 8, 3]
ENV = ("MCRAT_HIP_RANK_BLOCK", "MCRAT_HIP_RANK_FUSE", "MCRAT_HIP_NO_LDS_LISTS", "MCRAT_HIP_RANK_LAUNCH_CAP", "MCRAT_HIP_NO_COVERED", "MCRAT_HIP_HOST_GRID")
# threads per list, fused pass, columns in LDS
FORMS = {"256-fused-resident": (256, 1, 1), "256-unfused-resident": (256, 0, 1), "256-fused-columns-in-hbm": (256, 1, 0),
         "256-unfused-columns-in-hbm": (256, 0, 0), "128": (128, 0, 1)}
MESHES = {"cfg2": list(FORMS), "cut": list(FORMS), "2.5d": ["256-fused-resident", "256-unfused-resident"],
          "3d-polar-stokes": ["256-fused-resident", "256-unfused-columns-in-hbm"],
          # at lumi = 1e54 a pass is an event and few slots change cell, so the lookups are the forced pass's; on the benchmark's thin frame
          # (3e50) most slots change cell in every pass and the passes are fused ones
          "cfg2-thin": ["256-fused-resident", "256-fused-columns-in-hbm"], "cut-thin": ["256-fused-resident", "256-unfused-resident"]}


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def _make(mesh):
    n = sum(RAGGED)
    if mesh in ("cfg2", "cfg2-thin"):
        return synth.config2(n_photons=n, nzc=8, stokes=0, lumi=1e54 if mesh == "cfg2" else 3e50)
    if mesh in ("cut", "cut-thin"):
        return cut_mesh(n, lumi=1e54 if mesh == "cut" else 3e50)
    if mesh == "2.5d":
        return synth.config_25d(n_photons=n, stokes=1, lumi=1e54)
    return synth.config_3d(synth.POLAR, n_photons=n, stokes=1)


def _set_form(monkeypatch, block, fuse, lds, no_covered=False):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MCRAT_HIP_RANK_BLOCK", str(block))
    monkeypatch.setenv("MCRAT_HIP_RANK_FUSE", str(fuse))
    if not lds:
        monkeypatch.setenv("MCRAT_HIP_NO_LDS_LISTS", "1")
    if no_covered:
        monkeypatch.setenv("MCRAT_HIP_NO_COVERED", "1")


def _stats(st, rst):
    return tuple(getattr(st, k) for k in STAT_KEYS if k != "last_scattered_index" or rst.frame_scatt_cnt > 0)


@pytest.fixture(scope="module")
def cases(oracle):
    """per mesh, computed once: frame, cfg, the lists, and every list alone through the oracle's loop"""
    memo = {}

    def get(mesh):
        if mesh not in memo:
            frame, ph, cfg = _make(mesh)
            subs = _lists(ph, RAGGED)
            t0, rem = 0.5, 2.0 / frame["fps"]
            H = oracle.OracleHydro(frame)
            c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
            want = []
            for r, sub in enumerate(subs):
                P = oracle.OraclePhotons(synth.photons_to_aos(sub, oracle.PHOTON_DTYPE))
                rst, rtn, _, _ = oracle.photon_loop(c, P, H, seed=SEEDS[r], time_now=t0, remaining_time=rem, max_iterations=PASSES, stream=STREAMS[r])
                want.append((P.aos.copy(), rst, rtn))
            moved = sum(w[1].num_photons_find_new_element for w in want) / max(1, sum((w[1].iterations - 1) * n for w, n in zip(want, RAGGED)))
            print("%s: passes %s, events %s, not found %s, %.2f of the slots re-located per non-forced pass"
                  % (mesh, [w[1].iterations for w in want], [w[1].frame_scatt_cnt for w in want], [w[1].not_found for w in want], moved))
            assert sum(w[1].frame_scatt_cnt for w in want) > 0 and (moved > 0.5 or not mesh.endswith("-thin"))
            memo[mesh] = (frame, cfg, subs, t0, rem, want)
        return memo[mesh]
    return get


def _run_pool(hip, frame, cfg, subs, t0, rem):
    """the lists as a rank pool -> (the table's covered share, [(records, statistics)])"""
    pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    try:
        pool.set_hydro(frame)
        table = pool.covered_octants()
        pool.pool_create(len(subs), 1024)
        for r, sub in enumerate(subs):
            v = pool.pool_rank(r, STREAMS[r])
            v.set_photons(sub)
            v.begin_frame(SEEDS[r], t0, rem)
        pool.run(PASSES)
        out = []
        for r in range(len(subs)):
            v = pool.pool_rank(r, STREAMS[r])
            out.append((v.get_photons(), v.frame_statistics()))
        return table, out
    finally:
        pool.close()


def _same_bytes(a, b, what):
    for (pa, sa), (pb, sb) in zip(a, b):
        assert sorted(pa.keys()) == sorted(pb.keys())
        for k in pa:
            assert np.asarray(pa[k]).tobytes() == np.asarray(pb[k]).tobytes(), (what, k)
        assert all(getattr(sa, k) == getattr(sb, k) for k in STAT_KEYS) and sa.time_now == sb.time_now, what


# ---------------------------------------------------------------- the table itself

@pytest.mark.parametrize("mesh", ["cfg2", "3d-polar-stokes", "cut"])
def test_device_built_table_equals_host_built(hip, monkeypatch, mesh):
    frame, _, cfg = _make(mesh)
    got, size = {}, {}
    for how in ("device", "host", "off"):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        if how == "host":
            monkeypatch.setenv("MCRAT_HIP_HOST_GRID", "1")
        if how == "off":
            monkeypatch.setenv("MCRAT_HIP_NO_COVERED", "1")
        e = hip.Engine(cfg["dimensions"], cfg["geometry"], 0)
        try:
            e.set_hydro(frame)
            got[how] = e.covered_octants()
            size[how] = e.device_bytes()
        finally:
            e.close()
    nocts = 8 if cfg["dimensions"] == synth.THREE else 4
    t = got["device"]
    print("%s: %d entries, %d covered (%.3f)" % (mesh, t.size, np.count_nonzero(t >= 0), np.count_nonzero(t >= 0) / max(1, t.size)))
    assert t.size > 0 and t.size % nocts == 0
    assert np.array_equal(t, got["host"])
    assert t.min() >= -1 and t.max() < frame["num_elements"] and np.count_nonzero(t >= 0) > 0.25 * t.size
    if mesh == "cut":
        assert np.count_nonzero(t < 0) > 0.25 * t.size
    assert got["off"].size == 0
    # the table is part of the grid's allocation, behind the 256-B rule, and counted
    assert size["device"] - size["off"] == (4 * t.size + 255) // 256 * 256


def test_cut_mesh_mixes_covered_and_uncovered_slots_in_a_wave(driver):
    """the premise of the `cut` cases, on the host: of the 1000-photon list's and of the 300-photon list's first 128 slots (a wave's first trip of
    the fused pass: two slots per thread) some start in a covered quadrant and some do not; on the uncut mesh all but the few at a face do"""
    for mesh, lo, hi in (("cut", 0.05, 0.95), ("cfg2", 0.99, 1.01)):
        frame, ph, _ = _make(mesh)
        a0 = np.sqrt(ph["r0"] * ph["r0"] + ph["r1"] * ph["r1"])       # physics.hpp, hydro_coords, 2-D cylindrical
        got = run_mesh(driver, "mix_" + mesh, frame_columns(frame), n_seeded=10, n_octants=10, points=[a0, np.asarray(ph["r2"], dtype=np.float64)])
        flags, first = got["flags"], np.cumsum([0] + RAGGED)
        assert flags.size == sum(RAGGED)
        for r in (3, 4):
            share = float(np.mean(flags[first[r]:first[r] + 128]))
            print("%s, list of %d: %.2f of its first 128 slots start in a covered quadrant" % (mesh, RAGGED[r], share))
            assert lo < share < hi


# ---------------------------------------------------------------- parity, rank pool

@pytest.mark.parametrize("mesh,form", [(m, f) for m in MESHES for f in MESHES[m]])
def test_ragged_lists(hip, cases, monkeypatch, mesh, form):
    frame, cfg, subs, t0, rem, want = cases(mesh)
    _set_form(monkeypatch, *FORMS[form])
    table, on = _run_pool(hip, frame, cfg, subs, t0, rem)
    assert table.size > 0 and np.count_nonzero(table >= 0) > 0
    for r, ((recs, st), (ref, rst, rtn)) in enumerate(zip(on, want)):
        assert _stats(st, rst) == _stats(rst, rst), (mesh, form, r)
        assert st.time_now == pytest.approx(rtn, rel=1e-12), (mesh, form, r)
        try:
            _compare(recs, ref)
        except AssertionError as err:
            raise AssertionError("%s, %s, list %d: %s" % (mesh, form, r, err))
    _set_form(monkeypatch, *FORMS[form], no_covered=True)
    table_off, off = _run_pool(hip, frame, cfg, subs, t0, rem)
    assert table_off.size == 0
    _same_bytes(on, off, (mesh, form))


# ---------------------------------------------------------------- the frame queue

@pytest.mark.parametrize("mesh", ["cfg2", "cut"])
def test_through_the_frame_queue(hip, oracle, monkeypatch, mesh):
    """two chained frames in one queue launch, the 63-photon list joins at frame 1 (whole frames: the queue takes no pass limit -- a few thousand
    passes of the longest list, an event in nearly every one)"""
    frame, ph, cfg = _make(mesh)
    subs = _lists(ph, RAGGED)
    R, F, late = len(RAGGED), 2, 1
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
            rst, t, _, _ = oracle.photon_loop(c, P, H, seed=int(seeds[f][r]), time_now=t, remaining_time=ends[f] - t, stream=STREAMS[r])
            row.append((P.aos.copy(), rst, t))
        want.append(row)
    open_ = np.ones((F, R), dtype=np.int32)
    open_[0][late] = 0
    frame_end = np.array([[ends[f]] * R for f in range(F)])
    last = {}
    for fuse, no_covered in ((1, False), (0, False), (1, True)):
        _set_form(monkeypatch, 256, fuse, 1, no_covered=no_covered)
        pool = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], profile=True)
        pool.set_hydro(frame)
        assert (pool.covered_octants().size == 0) == no_covered
        pool.pool_create(R, 1024)
        stride = pool.n // R
        for r in range(R):
            pool.pool_rank(r, STREAMS[r]).set_photons(subs[r])
        got = pool.pool_run_frames(open_, seeds, np.zeros((F, R)), frame_end.copy(), frame_end=frame_end, chain_clock=True, capture=True)
        try:
            assert got[0][0].step_kernel_launches == 1, ("the plan did not run as one queue launch", got[0][0].step_kernel_launches)
            recs_all = {}
            for f in range(F):
                pool.pool_select_frame(f if f < F - 1 else -1)
                for r in range(R):
                    if want[r][f] is None:
                        assert got[f][r].iterations == 0
                        continue
                    ref, rst, rtn = want[r][f]
                    what = "%s, fuse %d, table off %s, frame %d, list %d" % (mesh, fuse, no_covered, f, r)
                    assert _stats(got[f][r], rst) == _stats(rst, rst), what
                    assert got[f][r].time_now == pytest.approx(rtn, rel=1e-12), what
                    recs = pool.get_photons_range(r * stride, RAGGED[r]) if f < F - 1 else pool.views[r].get_photons()
                    try:
                        _compare(recs, ref)
                    except AssertionError as err:
                        raise AssertionError("%s: %s" % (what, err))
                    recs_all[(f, r)] = {k: np.asarray(recs[k]).tobytes() for k in (recs.keys() if hasattr(recs, "keys") else recs.dtype.names)}
            last[(fuse, no_covered)] = recs_all
        finally:
            pool.pool_select_frame(-1)
            pool.close()
    assert last[(1, False)] == last[(1, True)]


# ---------------------------------------------------------------- list mode: step_kernel

def test_list_mode_step_kernel(hip, cases, monkeypatch):
    frame, cfg, subs, t0, rem, want = cases("cut")
    r = 4
    out = {}
    for no_covered in (False, True):
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        if no_covered:
            monkeypatch.setenv("MCRAT_HIP_NO_COVERED", "1")
        e = hip.Engine(cfg["dimensions"], cfg["geometry"], cfg["stokes"], rng_stream=STREAMS[r])
        try:
            e.set_hydro(frame)
            assert (e.covered_octants().size == 0) == no_covered
            e.set_photons(subs[r])
            e.begin_frame(SEEDS[r], t0, rem)
            st = e.run(PASSES)
            out[no_covered] = (e.get_photons(), st)
        finally:
            e.close()
    _same_bytes([out[False]], [out[True]], "list mode")
    recs, st = out[False]
    ref, rst, rtn = want[r]
    assert _stats(st, rst) == _stats(rst, rst)
    assert st.time_now == pytest.approx(rtn, rel=1e-12)
    _compare(recs, ref)
