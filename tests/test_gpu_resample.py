"""Resampled sky observations on the device (mcrat_hip_observe_sky_resampled, mcrat_hip_pool_observe_sky_resampled; mcrat_amd/csrc/resample.hip)
against the NumPy restatement of the definitions in tests/resample_checker.py (itself held to closed forms in tests/test_resample_checker_cpu.py).

count and the three per-observer counters must be EXACTLY equal on all three accumulation paths: the multiplicities are integer arithmetic and every
expression that decides a bin is bit-identical on the device and in the checker.  Each of the six sums of a bin must be within
(m + 2) * 2**-53 * sum|k * term| of the checker's fsum of the bin's m terms k * term (resample_checker.compare): the project's bound for sums added in
any order, here with the terms as the device adds them -- the rotated (Q, U) are bit-identical too.

The eight-photon ring about the axis: at a finite polar angle alpha the rotated Q' of the eight do not sum to 0 but to
4 sin^2 alpha / (1 + cos^2 alpha) (2e-8 at alpha = 1e-4; tests/test_resample_checker_cpu.py, ring_q_sum), so Q' is held to that closed form and U' to
0 within the rounding bound, and to 0 itself at alpha = 1e-9 where the closed form is below the bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from mcrat_amd import synth
from tests import resample_checker as R
from tests import sky_checker as S
from tests import test_resample_plan_cpu as RP
from tests.test_gpu_sky import _abi_observer, cut, placed
from tests.test_resample_checker_cpu import ring_q_sum

pytestmark = pytest.mark.gpu

PATHS = ("lds", "sliced", "global")
TIME_NOW = 400.0
# two observers off the axis at different azimuths whose cones overlap
OBSERVERS = S.observers([0.25, 0.3], [0.3, 1.2], [0.25, 0.25])
T_EDGES = np.linspace(100.0, 360.0, 4)                 # some photons fall outside (tests/test_gpu_sky.py)
E_EDGES = 10.0 ** np.linspace(-9.0, -4.0, 3)
X_EDGES = np.array([-3.0e12, 0.0, 3.0e12])             # 2 x 2 pixels
Y_EDGES = np.array([-2.0e12, 0.0, 2.0e12])
AXIS = (np.array([[0.0], [0.0], [1.0]]), np.array([math.cos(0.1)]), np.array([[1.0], [0.0], [0.0]]), np.array([[0.0], [1.0], [0.0]]))
WIDE_T, WIDE_E = np.array([-1e9, 1e9]), np.array([1e-300, 1e300])
LDS_BUDGET = 80 * 1024


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def engine_with(hip, ph, stokes=1):
    e = hip.Engine(synth.TWO, synth.CYLINDRICAL, stokes)
    e.set_photons(ph)
    return e


@functools.lru_cache(maxsize=None)
def base():
    """257 photons of a jet that is not axisymmetric (shared by the tests: do not change it)"""
    return S.jet_photons(101, 257)


def edges_of(image):
    return (T_EDGES, E_EDGES, X_EDGES, Y_EDGES) if image else (T_EDGES, E_EDGES, None, None)


def observe(e, obs, time_now, mode, n_rep, frame, seed, image, pool=False, edges=None):
    n, cos_acc, ex, ey = obs
    te, ee, xe, ye = edges or edges_of(image)
    f = e.pool_observe_sky_resampled if pool else e.observe_sky_resampled
    return f(n, cos_acc, te, ee, time_now, mode, n_rep, frame, seed, ex, ey, xe, ye)


def want_of(ph, obs, time_now, mode, n_rep, frame, seed, image, rank=0, slot=None, stokes=True, edges=None):
    n, cos_acc, ex, ey = obs
    te, ee, xe, ye = edges or edges_of(image)
    return R.observation(ph, n, cos_acc, te, ee, time_now, mode, n_rep, frame, seed, rank, slot, ex, ey, xe, ye, stokes=stokes)


def fitting_paths(n_obs, n_rep, n_t, n_e, n_x, n_y, axes=True):
    """the paths that may be forced for a cube (the header's layout: 7 planes of 8 bytes; the staged doubles and three counters per observer)"""
    image = n_x > 0
    staged = 8 * ((10 if axes else 4) * n_obs + n_t + 1 + n_e + 1 + (n_x + n_y + 2 if image else 0)) + 24 * n_obs
    replica = 56 * n_obs * n_t * n_e * max(n_x, 1) * max(n_y, 1)
    return [p for p, need in (("lds", staged + n_rep * replica), ("sliced", staged + replica), ("global", 0)) if need <= LDS_BUDGET]


def path_number(hip, path):
    return {"lds": hip.RESAMPLE_PATH_LDS, "sliced": hip.RESAMPLE_PATH_SLICED, "global": hip.RESAMPLE_PATH_GLOBAL}[path]


def on_every_path(hip, monkeypatch, e, paths, call):
    """call() under each forced path -> {path: result}; the path that ran is the one reported; the counts of all paths are equal"""
    got = {}
    for path in paths:
        monkeypatch.setenv("MCRAT_HIP_RESAMPLE_PATH", path)
        got[path] = call()
        assert e.observe_sky_resampled_path() == path_number(hip, path)
    first = got[paths[0]]
    for path in paths[1:]:
        for k in R.COUNTERS + ("count",):
            assert np.array_equal(first[k], got[path][k]), (path, k)
    return got


# ---------------------------------------------------------------------------------------------- 1: modes, replicas, frames, images, paths
MODES = [(R.NONE, 1), (R.JACKKNIFE, 2), (R.JACKKNIFE, 3), (R.JACKKNIFE, 64), (R.BOOTSTRAP, 2), (R.BOOTSTRAP, 3), (R.BOOTSTRAP, 5), (R.BOOTSTRAP, 6),
         (R.BOOTSTRAP, 64)]


@pytest.mark.parametrize("image", [False, True])
@pytest.mark.parametrize("frame", [R.AS_STORED, R.SKY_PLANE])
@pytest.mark.parametrize("mode,n_rep", MODES)
def test_counts_and_sums_on_every_path(hip, monkeypatch, mode, n_rep, frame, image):
    ph = base()
    paths = fitting_paths(2, n_rep, 3, 2, 2 if image else 0, 2 if image else 0)
    assert "sliced" in paths and "global" in paths and (("lds" in paths) == (n_rep < 64 or not image))
    want = want_of(ph, OBSERVERS, TIME_NOW, mode, n_rep, frame, 20260101, image)
    e = engine_with(hip, ph)
    assert e.observe_sky_resampled_path() == 0
    got = on_every_path(hip, monkeypatch, e, paths, lambda: observe(e, OBSERVERS, TIME_NOW, mode, n_rep, frame, 20260101, image))
    for path, res in got.items():
        assert res["count"].shape == ((2, n_rep, 3, 2, 2, 2) if image else (2, n_rep, 3, 2))
        R.compare(res, want, "mode %d n_rep %d frame %d image %d %s" % (mode, n_rep, frame, image, path))
    acc = S.per_photon(ph, OBSERVERS[0], OBSERVERS[1], T_EDGES, E_EDGES, TIME_NOW)["accepted"]
    assert (acc.sum(axis=1) > 20).all() and (acc[0] & acc[1]).sum() > 5 and (want["n_outside"] > 0).all()       # the cones overlap; some fall outside
    assert (want["n_frame_undefined"] == 0).all()
    if frame == R.SKY_PLANE:                                              # the rotation matters off the axis
        stored = want_of(ph, OBSERVERS, TIME_NOW, mode, n_rep, R.AS_STORED, 20260101, image)
        assert np.abs(stored["q"] - want["q"]).max() > 1e-3 * np.abs(want["q"]).max() and np.array_equal(stored["i"], want["i"])
    e.close()


# ---------------------------------------------------------------------------------------------- 2: list lengths
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_list_lengths(hip, monkeypatch, n):
    ph = cut(base(), n)
    e = engine_with(hip, ph)
    for mode, n_rep in ((R.BOOTSTRAP, 6), (R.JACKKNIFE, 3)):
        want = want_of(ph, OBSERVERS, TIME_NOW, mode, n_rep, R.SKY_PLANE, 5, True)
        got = on_every_path(hip, monkeypatch, e, PATHS, lambda: observe(e, OBSERVERS, TIME_NOW, mode, n_rep, R.SKY_PLANE, 5, True))
        for path, res in got.items():
            R.compare(res, want, "n=%d mode %d %s" % (n, mode, path))
    e.close()


# ---------------------------------------------------------------------------------------------- 3: against observe_sky
@pytest.mark.parametrize("image", [False, True])
def test_against_observe_sky(hip, monkeypatch, image):
    ph = base()
    e = engine_with(hip, ph)
    n, cos_acc, ex, ey = OBSERVERS
    te, ee, xe, ye = edges_of(image)
    monkeypatch.delenv("MCRAT_HIP_SKY_PATH", raising=False)
    sky = e.observe_sky(n, cos_acc, te, ee, TIME_NOW, ex if image else None, ey if image else None, xe, ye)
    sky_want = S.observation(ph, n, cos_acc, te, ee, TIME_NOW, ex if image else None, ey if image else None, xe, ye)
    assert sky["count"].sum() > 50
    # NONE / AS_STORED: the sky observation itself -- counts and counters exactly, the sums within twice its bound
    for path, res in on_every_path(hip, monkeypatch, e, PATHS, lambda: observe(e, OBSERVERS, TIME_NOW, R.NONE, 1, R.AS_STORED, 0, image)).items():
        assert np.array_equal(res["count"][:, 0], sky["count"]) and np.array_equal(res["n_accepted"], sky["n_accepted"])
        assert np.array_equal(res["n_outside"], sky["n_outside"]) and not res["n_frame_undefined"].any()
        for k, _ in S.PLANES:
            bound = 2.0 * (sky_want["count"] + 2.0) * S.U * sky_want["abs_" + k]
            assert (np.abs(res[k][:, 0] - sky[k]) <= bound).all(), (path, k)
    # JACKKNIFE: the groups are disjoint and together the sample
    for G in (2, 5, 64):
        for path, res in on_every_path(hip, monkeypatch, e, fitting_paths(2, G, 3, 2, 2 * image, 2 * image),
                                       lambda: observe(e, OBSERVERS, TIME_NOW, R.JACKKNIFE, G, R.AS_STORED, 9, image)).items():
            assert np.array_equal(res["count"].sum(axis=1), sky["count"]), (G, path)
            assert (res["count"].sum(axis=tuple(range(2, res["count"].ndim))) > 0).sum() > 2                 # more than one group is in use
    # BOOTSTRAP: entry 0 is the sample; no entry holds more than 12 times it
    for n_rep in (2, 6, 64):
        for path, res in on_every_path(hip, monkeypatch, e, fitting_paths(2, n_rep, 3, 2, 2 * image, 2 * image),
                                       lambda: observe(e, OBSERVERS, TIME_NOW, R.BOOTSTRAP, n_rep, R.AS_STORED, 9, image)).items():
            assert np.array_equal(res["count"][:, 0], sky["count"]), (n_rep, path)
            assert (res["count"] <= 12 * sky["count"][:, None]).all() and (res["count"][:, 1:] != sky["count"][:, None]).any()
    e.close()


# ---------------------------------------------------------------------------------------------- 4: a pool of three ragged lists
def ragged_lists():
    lens = [65, 1, 191]
    starts = np.concatenate([[0], np.cumsum(lens)])
    lists = [cut(base(), int(a), int(b)) for a, b in zip(starts[:-1], starts[1:])]
    kind = np.random.default_rng(8).integers(0, 6, lens[2])
    lists[2]["weight"][kind == 0] = 0.0
    lists[2]["type"][kind == 1] = b"p"
    lists[2]["type"][kind == 2] = b"N"
    assert all((kind == k).sum() > 10 for k in (0, 1, 2))
    return lens, lists


@pytest.mark.parametrize("mode,n_rep", [(R.NONE, 1), (R.JACKKNIFE, 5), (R.BOOTSTRAP, 6), (R.BOOTSTRAP, 64)])
def test_pool_equals_its_views(hip, monkeypatch, mode, n_rep):
    lens, lists = ragged_lists()
    ranks, clocks = [0, 2, 3], np.array([400.0, -1.0e9, 380.0, 410.0])      # rank 1 is never created
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(4, 200)
    for r, ph in zip(ranks, lists):
        pool.pool_rank(r, r).set_photons(ph)
    everything = S.concatenate(lists)
    tn = np.concatenate([np.full(m, clocks[r]) for r, m in zip(ranks, lens)])
    rank = np.concatenate([np.full(m, r) for r, m in zip(ranks, lens)])
    slot = np.concatenate([np.arange(m) for m in lens])
    want = want_of(everything, OBSERVERS, tn, mode, n_rep, R.SKY_PLANE, 77, True, rank=rank, slot=slot)
    paths = fitting_paths(2, n_rep, 3, 2, 2, 2)                            # 64 entries: three slices, and the pool's four workgroups shared among them
    got = on_every_path(hip, monkeypatch, pool, paths, lambda: observe(pool, OBSERVERS, clocks, mode, n_rep, R.SKY_PLANE, 77, True, pool=True))
    for path, res in got.items():
        R.compare(res, want, "pool mode %d %s" % (mode, path))
    assert want["count"].sum() > 50
    if mode != R.NONE:                                                    # the identity is (rank, slot), not the pool-wide index
        other = want_of(everything, OBSERVERS, tn, mode, n_rep, R.SKY_PLANE, 77, True)
        assert not np.array_equal(other["count"], want["count"])
    # each view alone: that list with the same multiplicities; together they are the pool's counts
    monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
    alone = []
    for r, ph in zip(ranks, lists):
        alone.append(observe(pool.pool_rank(r, r), OBSERVERS, clocks[r], mode, n_rep, R.SKY_PLANE, 77, True))
        R.compare(alone[-1], want_of(ph, OBSERVERS, clocks[r], mode, n_rep, R.SKY_PLANE, 77, True, rank=r), "view %d" % r)
    for k in R.COUNTERS + ("count",):
        assert np.array_equal(sum(a[k] for a in alone), got[paths[0]][k]), k
    pool.close()


# ---------------------------------------------------------------------------------------------- 5: seeds
def test_seeds(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
    e = engine_with(hip, base())
    for mode, n_rep in ((R.JACKKNIFE, 8), (R.BOOTSTRAP, 9)):
        a, b = (observe(e, OBSERVERS, TIME_NOW, mode, n_rep, R.AS_STORED, 1234, False) for _ in range(2))
        c = observe(e, OBSERVERS, TIME_NOW, mode, n_rep, R.AS_STORED, 1235, False)
        d = observe(e, OBSERVERS, TIME_NOW, mode, n_rep, R.AS_STORED, 1234 + (1 << 32), False)      # the seed's upper half counts
        assert np.array_equal(a["count"], b["count"]) and not np.array_equal(a["count"], c["count"]) and not np.array_equal(a["count"], d["count"])
        R.compare(d, want_of(base(), OBSERVERS, TIME_NOW, mode, n_rep, R.AS_STORED, 1234 + (1 << 32), False), "upper seed", exact_only=True)
    e.close()


# ---------------------------------------------------------------------------------------------- 6: SKY_PLANE in closed form
def test_ring_about_the_axis(hip, monkeypatch):
    az = np.arange(8) * (math.pi / 4)
    bound = 8 * 10 * 2.0 ** -53 + (8 + 2) * 2.0 ** -53 * 8                # tests/test_resample_checker_cpu.py, check_ring_about_the_axis
    for alpha, q_sum in ((1e-4, ring_q_sum(1e-4)), (1e-9, 0.0)):
        ph = R.ring_photons(alpha, az)
        e = engine_with(hip, ph)
        got = on_every_path(hip, monkeypatch, e, PATHS, lambda: observe(e, AXIS, TIME_NOW, R.NONE, 1, R.SKY_PLANE, 0, False, edges=(WIDE_T, WIDE_E, None, None)))
        want = want_of(ph, AXIS, TIME_NOW, R.NONE, 1, R.SKY_PLANE, 0, False, edges=(WIDE_T, WIDE_E, None, None))
        for path, res in got.items():
            R.compare(res, want, "ring %g %s" % (alpha, path))
            assert res["count"].item() == 8 and res["n_frame_undefined"].tolist() == [0]
            assert abs(res["q"].item() - q_sum) <= bound and abs(res["u"].item()) <= bound, (alpha, path, res["q"].item(), res["u"].item())
            assert res["i"].item() == 8.0 == res["w"].item()
        stored = observe(e, AXIS, TIME_NOW, R.NONE, 1, R.AS_STORED, 0, False, edges=(WIDE_T, WIDE_E, None, None))
        assert stored["q"].item() == 8.0 == stored["w"].item() and stored["u"].item() == 0.0          # full polarisation where the sky-plane sum is none
        e.close()


def test_undefined_frames_are_counted_and_added_as_stored(hip, monkeypatch):
    ph = S.concatenate([R.ring_photons(0.0, [0.0, 1.0, 2.0], Q=0.25, Uq=-0.5), R.ring_photons(0.05, [0.7, 2.9], Q=0.25, Uq=-0.5)])
    ph["p3"][1] = -ph["p3"][1]                                            # along -z_hat: undefined, but no observer accepts it
    two = tuple(np.concatenate([a, a], axis=-1) for a in AXIS)            # the same observer twice: both count the pair
    want = want_of(ph, two, TIME_NOW, R.BOOTSTRAP, 4, R.SKY_PLANE, 3, False, edges=(WIDE_T, WIDE_E, None, None))
    assert want["n_frame_undefined"].tolist() == [2, 2] and want["n_accepted"].tolist() == [4, 4]
    e = engine_with(hip, ph)
    for path, res in on_every_path(hip, monkeypatch, e, PATHS,
                                   lambda: observe(e, two, TIME_NOW, R.BOOTSTRAP, 4, R.SKY_PLANE, 3, False, edges=(WIDE_T, WIDE_E, None, None))).items():
        R.compare(res, want, "undefined " + path)
    e.close()
    off = engine_with(hip, ph, stokes=0)                                  # nothing to rotate: nothing undefined
    monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
    res = observe(off, two, TIME_NOW, R.BOOTSTRAP, 4, R.SKY_PLANE, 3, False, edges=(WIDE_T, WIDE_E, None, None))
    assert res["n_frame_undefined"].tolist() == [0, 0] and np.array_equal(res["count"], want["count"])
    off.close()


# ---------------------------------------------------------------------------------------------- 7: contention, Stokes off
def test_all_photons_in_one_bin(hip, monkeypatch):
    ph = placed(100.0 * S.C_LIGHT, np.full(257, 5e9), np.full(257, 5e9))
    edges = (np.array([200.0, 400.0]), np.array([1e-12, 1e-3]), np.array([0.0, 1e10]), np.array([0.0, 1e10]))
    obs = (AXIS[0], np.array([0.5]), AXIS[2], AXIS[3])
    e = engine_with(hip, ph)
    for mode, n_rep in ((R.NONE, 1), (R.JACKKNIFE, 2), (R.BOOTSTRAP, 5)):
        want = want_of(ph, obs, TIME_NOW, mode, n_rep, R.AS_STORED, 11, True, edges=edges)
        assert want["count"].sum() >= 257 and want["n_outside"].tolist() == [0]
        for path, res in on_every_path(hip, monkeypatch, e, PATHS, lambda: observe(e, obs, TIME_NOW, mode, n_rep, R.AS_STORED, 11, True, edges=edges)).items():
            R.compare(res, want, "one bin mode %d %s" % (mode, path))
    e.close()


@pytest.mark.parametrize("frame", [R.AS_STORED, R.SKY_PLANE])
def test_stokes_off(hip, monkeypatch, frame):
    ph = base()
    off = engine_with(hip, ph, stokes=0)
    want = want_of(ph, OBSERVERS, TIME_NOW, R.BOOTSTRAP, 5, frame, 2, True, stokes=False)
    on = want_of(ph, OBSERVERS, TIME_NOW, R.BOOTSTRAP, 5, frame, 2, True)
    for path, res in on_every_path(hip, monkeypatch, off, PATHS, lambda: observe(off, OBSERVERS, TIME_NOW, R.BOOTSTRAP, 5, frame, 2, True)).items():
        R.compare(res, want, "stokes off " + path)
        for k in ("i", "q", "u", "v"):
            assert not res[k].any() and on[k].any()
        assert np.array_equal(res["count"], on["count"]) and res["w"].any()
    off.close()


# ---------------------------------------------------------------------------------------------- 8: one replica fits LDS, two do not
def test_slices_of_one_replica(hip, monkeypatch):
    """1 x 4 x 3 x 8 x 8 bins are 43 008 bytes a replica: one fits the 80 KiB beside the staged inputs, two do not -- three slices of one replica"""
    xe, ye = np.linspace(-4e12, 4e12, 9), np.linspace(-4e12, 4e12, 9)
    te, ee = np.linspace(100.0, 360.0, 5), 10.0 ** np.linspace(-9.0, -4.0, 4)
    assert fitting_paths(1, 3, 4, 3, 8, 8) == ["sliced", "global"] and fitting_paths(1, 2, 4, 3, 8, 8) == ["sliced", "global"]
    obs = tuple(a[..., :1] for a in OBSERVERS)
    ph = base()
    e = engine_with(hip, ph)
    for mode in (R.JACKKNIFE, R.BOOTSTRAP):
        want = want_of(ph, obs, TIME_NOW, mode, 3, R.SKY_PLANE, 8, True, edges=(te, ee, xe, ye))
        got = on_every_path(hip, monkeypatch, e, ["sliced", "global"], lambda: observe(e, obs, TIME_NOW, mode, 3, R.SKY_PLANE, 8, True, edges=(te, ee, xe, ye)))
        for path, res in got.items():
            R.compare(res, want, "slices mode %d %s" % (mode, path))
        assert (want["count"].sum(axis=(0, 2, 3, 4, 5)) > 0).all()            # every slice has something to flush
        monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
        R.compare(observe(e, obs, TIME_NOW, mode, 3, R.SKY_PLANE, 8, True, edges=(te, ee, xe, ye)), want, "slices, the rule", exact_only=True)
        assert e.observe_sky_resampled_path() == hip.RESAMPLE_PATH_SLICED
    e.close()


# ---------------------------------------------------------------------------------------------- 9: refusals and states through the ABI
def test_refusals_reach_the_caller(hip, monkeypatch):
    e = engine_with(hip, cut(base(), 10))
    lib = e.lib
    def call(c, ctx=e):
        keep = []
        obs = hip.ResampleObserver(_abi_observer(hip, c, keep), c["mode"], c["n_rep"], c["frame"], 1)
        out = hip.ResampleObservation()
        return lib.mcrat_hip_observe_sky_resampled(ctx.ctx, C.byref(obs), TIME_NOW, C.byref(out)), obs, out, keep
    for name, why in sorted(RP.REFUSED.items()):
        c = RP.PLANS[name]
        if c["env"] is None:
            monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
        else:
            monkeypatch.setenv("MCRAT_HIP_RESAMPLE_PATH", c["env"])
        assert call(c)[0] == -1, name                                     # MCRAT_HIP_EINVAL
        assert lib.mcrat_hip_last_error(e.ctx).decode() == RP.TEXTS[why], name
        assert e.observe_sky_resampled_path() == 0
    monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
    assert set(RP.OWN_CODES) <= set(RP.REFUSED.values())
    # through the Python interface
    with pytest.raises(hip.McratHipError, match="needs the sky-plane vectors"):
        e.observe_sky_resampled(AXIS[0], AXIS[1], T_EDGES, E_EDGES, TIME_NOW, stokes_frame=hip.STOKES_SKY_PLANE)
    with pytest.raises(hip.McratHipError, match="n_rep must be 1"):
        e.observe_sky_resampled(AXIS[0], AXIS[1], T_EDGES, E_EDGES, TIME_NOW, mode=hip.RESAMPLE_NONE, n_rep=3)
    # NULL output pointers: the call runs and writes nowhere; then only one counter
    rc, obs, out, keep = call(RP.PLANS["image_sky_plane"])
    assert rc == 0 and e.observe_sky_resampled_path() == hip.RESAMPLE_PATH_LDS
    n_acc = np.full(1, -1, dtype=np.int64)
    out.n_accepted = n_acc.ctypes.data_as(C.POINTER(C.c_longlong))
    assert lib.mcrat_hip_observe_sky_resampled(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == 0
    assert n_acc[0] == S.per_photon(cut(base(), 10), AXIS[0], [0.5], [0.0, 1.0], [0.0, 1.0], TIME_NOW)["accepted"].sum() > 0
    assert lib.mcrat_hip_observe_sky_resampled(None, C.byref(obs), TIME_NOW, C.byref(out)) == -1
    assert lib.mcrat_hip_observe_sky_resampled(e.ctx, None, TIME_NOW, C.byref(out)) == -1
    assert lib.mcrat_hip_observe_sky_resampled(e.ctx, C.byref(obs), TIME_NOW, None) == -1 and lib.mcrat_hip_observe_sky_resampled_path(None) == 0
    obs.sky.t_edges = None
    assert lib.mcrat_hip_observe_sky_resampled(e.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == -1
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "observe_sky_resampled: a null array in mcrat_hip_resample_observer"
    # the wrong kind of context, and no photons: MCRAT_HIP_ESTATE
    rc, obs, out, keep = call(RP.PLANS["image"])
    assert rc == 0
    clocks = np.array([TIME_NOW, TIME_NOW])
    dp = C.POINTER(C.c_double)
    ESTATE = -5
    assert lib.mcrat_hip_pool_observe_sky_resampled(e.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == ESTATE
    assert lib.mcrat_hip_last_error(e.ctx).decode() == "pool_observe_sky_resampled: the context is no rank pool"
    assert lib.mcrat_hip_pool_observe_sky_resampled(e.ctx, C.byref(obs), None, C.byref(out)) == -1
    empty = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    assert lib.mcrat_hip_observe_sky_resampled(empty.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    empty.close()
    pool = hip.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 64)
    pool.pool_rank(0, 0).set_photons(cut(base(), 10))
    assert lib.mcrat_hip_observe_sky_resampled(pool.ctx, C.byref(obs), TIME_NOW, C.byref(out)) == ESTATE
    assert "mcrat_hip_pool_observe_sky_resampled" in lib.mcrat_hip_last_error(pool.ctx).decode()
    assert lib.mcrat_hip_pool_observe_sky_resampled(pool.ctx, C.byref(obs), clocks.ctypes.data_as(dp), C.byref(out)) == 0
    with pytest.raises(ValueError):
        pool.pool_observe_sky_resampled(AXIS[0], AXIS[1], T_EDGES, E_EDGES, [TIME_NOW])      # one clock per list
    pool.close()
    e.close()


# ---------------------------------------------------------------------------------------------- 10: the rule's paths, and nothing changes
def test_the_rule_picks_the_path_and_photons_are_left_as_they_were(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_RESAMPLE_PATH", raising=False)
    ph = base()
    e = engine_with(hip, ph)
    before = e.get_photons()
    observe(e, OBSERVERS, TIME_NOW, R.BOOTSTRAP, 6, R.SKY_PLANE, 1, True)
    assert e.observe_sky_resampled_path() == hip.RESAMPLE_PATH_LDS
    observe(e, OBSERVERS, TIME_NOW, R.BOOTSTRAP, 64, R.SKY_PLANE, 1, True)         # 2 x 64 x 24 bins of 56 bytes: 172 KB, three slices of 30 replicas
    assert e.observe_sky_resampled_path() == hip.RESAMPLE_PATH_SLICED
    # one replica of 1 x 2 x 2 x 32 x 32 bins is 229 KB: no replica fits
    edges = (np.array([60.0, 250.0, 380.0]), np.array([1e-10, 1e-7, 1e-3]), np.linspace(-4e12, 4e12, 33), np.linspace(-4e12, 4e12, 33))
    obs = tuple(a[..., :1] for a in OBSERVERS)
    res = observe(e, obs, TIME_NOW, R.JACKKNIFE, 3, R.SKY_PLANE, 1, True, edges=edges)
    assert e.observe_sky_resampled_path() == hip.RESAMPLE_PATH_GLOBAL
    R.compare(res, want_of(ph, obs, TIME_NOW, R.JACKKNIFE, 3, R.SKY_PLANE, 1, True, edges=edges), "no replica fits")
    for path in PATHS:
        monkeypatch.setenv("MCRAT_HIP_RESAMPLE_PATH", path)
        observe(e, OBSERVERS, TIME_NOW, R.JACKKNIFE, 4, R.SKY_PLANE, 1, False)
    after = e.get_photons()
    assert set(before) == set(after)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k
    est = hip.resampled_estimates(observe(e, OBSERVERS, TIME_NOW, R.JACKKNIFE, 4, R.SKY_PLANE, 1, False), hip.RESAMPLE_JACKKNIFE, reduce=("time", "energy"))
    assert est["pi"]["value"].shape == (2,) and (est["pi"]["stderr"] > 0).all() and (est["w"]["stderr"] > 0).all()
    e.close()
