"""The CPU restatement of FAST mode (oracle/oracle_fast.c, oracle_py.fast_frame) on its own: tests/test_gpu_fast_parity.py holds the device kernel
against it photon for photon, so it must not be pinned only by the kernel it checks.  Here: the clocks, the one case in which FAST mode and the
reference's event-driven loop are the same algorithm (one window, one photon, one tape of uniforms), the scattering rate in a uniform medium
against its closed form, the photons that do not take part (null slots, photons without weight, photons outside the cells), the keys of the
draws, and the decision margins the parity tests rely on."""
import ctypes as C

import numpy as np
import pytest

from mcrat_amd import synth


def _setup(oracle, frame, ph, cfg, **kw):
    H = oracle.OracleHydro(frame)
    P = oracle.OraclePhotons(synth.photons_to_aos(ph, oracle.PHOTON_DTYPE))
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True, **kw)
    return c, P, H


def _same_records(a, b):
    """every member of the photon records, bit for bit (the bytes between the members are nobody's)"""
    return all(np.array_equal(a[k].view("u1" if a[k].dtype.kind == "S" else "u%d" % a[k].dtype.itemsize),
                              b[k].view("u1" if b[k].dtype.kind == "S" else "u%d" % b[k].dtype.itemsize)) for k in a.dtype.names)


def _copy(ph):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ph.items()}


@pytest.fixture(scope="module")
def dense():
    return synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=1e54)


@pytest.fixture(scope="module")
def thin():
    return synth.config2(n_photons=2001, nzc=8, stokes=1, lumi=3e50)


@pytest.mark.parametrize("which", ["dense", "thin"])
@pytest.mark.parametrize("windows", [1, 3, 8, 9, 64])
def test_the_flights_of_a_photon_fill_the_frame(oracle, dense, thin, which, windows):
    frame, ph, cfg = dense if which == "dense" else thin
    c, P, H = _setup(oracle, frame, ph, cfg)
    rem = 1.0 / frame["fps"]
    _, cnt, _ = oracle.fast_frame(c, P, H, 99, 0, rem, windows)
    flown, passes = oracle.fast_frame.flown, oracle.fast_frame.passes
    assert (passes >= windows).all() and passes.max() == cnt.passes and int(passes.sum()) == cnt.photon_steps
    assert (np.abs(flown - rem) <= passes * np.spacing(rem)).all()              # a sum of `passes` terms: an ulp each at the most
    ns = P.aos["num_scatt"] - ph["num_scatt"]
    assert int(ns.sum()) == cnt.scatterings and (ns >= 0).all()
    # every pass ends a window, scatters or is rejected -- nothing else: `windows` windows per photon, no more
    inside = P.aos["nearest_block_index"] != -1
    assert inside.all()
    assert cnt.photon_steps == windows * len(ns) + cnt.scatterings + cnt.kn_rejections
    same = ns == 0                                                               # never scattered: flew straight for the whole frame
    assert same.sum() > (1500 if which == "thin" else 0)
    d = synth.C_LIGHT * rem
    for r, p in (("r0", "p1"), ("r1", "p2"), ("r2", "p3")):
        assert np.allclose(P.aos[r][same], ph[r][same] + d * ph[p][same] / ph["p0"][same], rtol=1e-12, atol=0), r
    if which == "thin" and windows >= 8:
        assert cnt.scatterings < 0.05 * len(ns)                                  # (the thin frame of the parity tests: flights end on window boundaries)


@pytest.mark.parametrize("case", ["cold-stokes", "hot"])
def test_one_window_and_one_photon_is_the_reference_loop(oracle, case):
    """own clock and list clock are the same clock: both walks read ONE tape of uniforms in the same order and must leave the same bytes"""
    if case == "cold-stokes":
        frame, ph, cfg = synth.config2(n_photons=40, nzc=8, stokes=1, lumi=1e54)
        rem = 1.0 / frame["fps"]
    else:                                                                        # T' > 1e7 K: Maxwell-Juettner electrons, Klein-Nishina rejections
        frame, ph, cfg = synth.config2(n_photons=40, nzc=8, stokes=0, lumi=1e54, r_inj=1e11)
        rem = 0.1 / frame["fps"]
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"])
    aos = synth.photons_to_aos(ph, oracle.PHOTON_DTYPE)
    events = rejections = 0
    for i in range(len(aos)):
        tape = np.random.default_rng(1000 + i).random(400_000)
        A, B = oracle.OraclePhotons(aos[i:i + 1]), oracle.OraclePhotons(aos[i:i + 1])
        _, cnt, _ = oracle.fast_frame(c, A, H, 0, 0, rem, 1, tape=tape)
        st, tn, left, _ = oracle.photon_loop(c, B, H, seed=0, time_now=0.0, remaining_time=rem, tape=tape)
        assert left == 0.0 and oracle.fast_frame.tape_pos == oracle.photon_loop.tape_pos > 0
        assert _same_records(A.aos, B.aos), i
        assert (cnt.scatterings, cnt.kn_rejections, cnt.passes, cnt.photon_steps, cnt.not_found) == \
               (st.frame_scatt_cnt, st.kn_rejections, st.iterations, st.photon_steps, st.not_found)
        # (the loop does not count the forced search of its first iteration, mclib.c:608-611; FAST mode counts every search that finds a cell)
        assert cnt.relocated == st.num_photons_find_new_element + 1
        assert abs(oracle.fast_frame.flown[0] - tn) <= cnt.passes * np.spacing(rem)
        events += cnt.scatterings
        rejections += cnt.kn_rejections
    assert events > 100 and (case != "hot" or rejections > 0)


@pytest.mark.parametrize("windows", [1, 8, 64])
def test_scattering_rate_in_a_uniform_medium_at_rest(oracle, windows):
    """cold electrons at rest, soft photons: the scatterings of a photon in the frame are Poisson with mean c dt n sigma_T, whatever the windows"""
    frame, ph, cfg = synth.config1(n_photons=20_000, n0=32, n1=32)
    M, n = frame["num_elements"], len(ph["p0"])
    n_e = 7.5e14                                                                 # c dt n sigma_T = 2.99
    frame["dens_lab"] = np.full(M, n_e * synth.M_P)
    frame["dens"] = frame["dens_lab"].copy()
    frame["gamma"] = np.ones(M)
    frame["temp"] = np.full(M, 1e3)
    # at rest to nine digits: with exactly v = 0 the reference's optical depth is 0/0 (the cosine between the photon and the flow,
    # optical_depth.c:46) and nothing ever scatters; with gamma = 1 the factor 1 - beta cos is exactly 1 for any direction of the flow
    frame["v0"] = np.full(M, 1e-9)
    frame["v1"] = np.zeros(M)
    ph = _copy(ph)
    soft = 1e-12 / synth.C_LIGHT / ph["p0"]                                      # 0.6 eV: h nu / m_e c^2 = 1e-6, Klein-Nishina = Thomson to 2e-6
    for k in ("p0", "p1", "p2", "p3", "comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        ph[k] = ph[k] * soft
    c, P, H = _setup(oracle, frame, ph, cfg)
    rem = 1.0 / frame["fps"]
    _, cnt, _ = oracle.fast_frame(c, P, H, 2024 + windows, 0, rem, windows)
    assert (P.aos["nearest_block_index"] != -1).all() and cnt.not_found == 0      # the photons stayed in the medium
    want = synth.C_LIGHT * rem * n_e * synth.THOM_X_SECT
    got = cnt.scatterings / n
    assert abs(got - want) < 4 * np.sqrt(want / n), (got, want)
    assert cnt.kn_rejections < 1e-4 * cnt.scatterings + 5
    ns = P.aos["num_scatt"] - ph["num_scatt"]
    assert abs(ns.var() - want) < 0.1 * want                                     # Poisson: variance = mean (4 sigma of the sample variance's own error is 4 %)


def _with_bystanders(ph):
    """null slots, photons a hair inside the outer boundary heading out, photons without weight that are not null (tests/test_gpu_fast_mode.py)"""
    ph = _copy(ph)
    n = len(ph["p0"])
    null = np.arange(0, n, 97)
    ph["weight"][null] = 0.0                                                     # setNullPhoton, photons.c:210-250
    ph["type"][null] = b"N"
    ph["nearest_block_index"][null] = -1
    far = np.setdiff1d(np.arange(5, n, 211), null)
    ph["r2"][far] = 2.49999e13
    ph["p3"][far] = np.abs(ph["p0"][far]); ph["p1"][far] = 0; ph["p2"][far] = 0
    ghost = np.setdiff1d(np.arange(3, n, 53), np.concatenate([null, far]))
    ph["weight"][ghost] = 0.0
    return ph, null, far, ghost


def test_null_weightless_and_outside_photons(oracle, dense):
    frame, ph0, cfg = dense
    ph, null, far, ghost = _with_bystanders(ph0)
    c, P, H = _setup(oracle, frame, ph, cfg)
    rem = 1.0 / frame["fps"]
    _, cnt, _ = oracle.fast_frame(c, P, H, 5, 0, rem, 8)
    out, flown, passes = P.aos, oracle.fast_frame.flown, oracle.fast_frame.passes
    # null slots: one pass (no cell: the frame is over at once), nothing changed but time_to_scatter, which calcMeanFreePath sets for every slot
    # of the list to the 1e12 cm of a photon without a cell (mclib.c:646,684-687)
    for k in oracle.PHOTON_DTYPE.names:
        if k != "time_to_scatter":
            assert np.array_equal(out[k][null], ph[k][null]), k
    assert (passes[null] == 1).all() and np.array_equal(out["time_to_scatter"][null], np.full(null.size, 1e12 / synth.C_LIGHT))
    # without weight but not null: stays where it is (mclib.c:1070) and scatters like any other photon
    for k in ("r0", "r1", "r2"):
        assert np.array_equal(out[k][ghost], ph[k][ghost]), k
    assert (out["num_scatt"][ghost] - ph["num_scatt"][ghost]).sum() > ghost.size
    assert (flown[ghost] > 0).all() and (np.abs(flown[ghost] - rem) <= passes[ghost] * np.spacing(rem)).all()
    # inside the domain but beyond the cells: not found (mclib.c:583), cell -1, the whole frame in one flight
    assert (out["nearest_block_index"][far] == -1).all() and cnt.not_found == far.size
    assert (passes[far] == 1).all() and np.array_equal(flown[far], np.full(far.size, rem))
    assert np.allclose(out["r2"][far], ph["r2"][far] + synth.C_LIGHT * rem, rtol=1e-15, atol=0)
    assert np.array_equal(out["weight"], ph["weight"]) and np.array_equal(out["type"], ph["type"])
    assert int((out["num_scatt"] - ph["num_scatt"]).sum()) == cnt.scatterings
    # a photon outside the DOMAIN loses its cell without a search
    ph2 = _copy(ph0)
    ph2["r2"][:10] = 2.6e13
    c, P, H = _setup(oracle, frame, ph2, cfg)
    _, cnt2, _ = oracle.fast_frame(c, P, H, 5, 0, rem, 8)
    assert (P.aos["nearest_block_index"][:10] == -1).all() and cnt2.not_found == 0 and (oracle.fast_frame.passes[:10] == 1).all()
    # no frame time, no frame
    c, P, H = _setup(oracle, frame, ph0, cfg)
    before = P.aos.copy()
    _, cnt3, _ = oracle.fast_frame(c, P, H, 5, 0, 0.0, 8)
    assert _same_records(P.aos, before) and cnt3.photon_steps == cnt3.passes == 0


def test_the_keys_of_the_draws(oracle, dense):
    """the free-path draw of slot i in pass p is words 0 and 1 of Philox{seed; p, i, purpose 8 | stream << 8}; a photon's frame depends on its slot
    number, the seed and the stream, and on nothing else in the list"""
    L = oracle.lib()
    rng = oracle.Rng()
    seed, stream, p, slot = 0x1234567890ABCDEF, 5, (7 << 32) | 11, 1023
    L.orc_rng_init(C.byref(rng), seed, stream)
    L.orc_rng_set_iteration(C.byref(rng), p)
    ctr = (C.c_uint32 * 4)(p & 0xffffffff, p >> 32, slot, 8 | (stream << 8))
    key = (C.c_uint32 * 2)(seed & 0xffffffff, seed >> 32)
    w = (C.c_uint32 * 4)()
    L.orc_philox4x32_10(ctr, key, w)
    bits = w[0] | (w[1] << 32)
    assert L.orc_rng_fast_freepath_draw(C.byref(rng), slot) == ((bits >> 12) + 0.5) * 2.0 ** -52
    frame, ph, cfg = dense
    rem = 1.0 / frame["fps"]
    aos = synth.photons_to_aos(ph, oracle.PHOTON_DTYPE)[:64]
    H = oracle.OracleHydro(frame)
    c = oracle.make_config(cfg["dimensions"], cfg["geometry"], cfg["stokes"], optimised=True)
    whole = oracle.OraclePhotons(aos)
    oracle.fast_frame(c, whole, H, 77, 3, rem, 8)
    part = oracle.OraclePhotons(aos[40:])
    oracle.fast_frame(c, part, H, 77, 3, rem, 8, slot_base=40)
    assert _same_records(part.aos, whole.aos[40:])
    for other in (dict(seed=78), dict(stream=4), dict(slot_base=41)):
        kw = dict(seed=77, stream=3, slot_base=40)
        kw.update(other)
        again = oracle.OraclePhotons(aos[40:])
        oracle.fast_frame(c, again, H, kw["seed"], kw["stream"], rem, 8, slot_base=kw["slot_base"])
        assert not np.array_equal(again.aos["p0"], part.aos["p0"]), other


def test_margins_are_reported(oracle, dense):
    """how close the walk came to turning a decision on one rounding: the flight test t < limit and the Klein-Nishina acceptance test"""
    frame, ph, cfg = dense
    c, P, H = _setup(oracle, frame, ph, cfg)
    rem = 1.0 / frame["fps"]
    _, cnt, mg = oracle.fast_frame(c, P, H, 99, 0, rem, 8)
    assert cnt.scatterings > 10_000
    # the smallest of N distances of uniforms from a bound is about 1/N: positive, and far below the distances themselves
    assert 0 < mg.flight < 1e-2 and 0 < mg.kn < 1e-2
    few = oracle.OraclePhotons(synth.photons_to_aos(ph, oracle.PHOTON_DTYPE)[:3])
    _, cnt, mg3 = oracle.fast_frame(c, few, H, 99, 0, rem, 8)
    assert mg3.flight >= mg.flight and mg3.kn >= mg.kn                            # the same three photons' decisions are among the list's
    # no decision taken, none reported
    ph_n = _copy(ph)
    ph_n["nearest_block_index"][:] = -1
    c, P, H = _setup(oracle, frame, ph_n, cfg)
    _, cnt, mg0 = oracle.fast_frame(c, P, H, 99, 0, rem, 8)
    assert cnt.scatterings == 0 and cnt.photon_steps == len(ph["p0"]) and mg0.flight > 1e300 and mg0.kn > 1e300
