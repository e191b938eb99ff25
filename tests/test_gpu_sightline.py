"""Line-of-sight optical depths and photospheres on the device (mcrat_hip_sightline_rays, mcrat_hip_sightline_photons,
mcrat_hip_pool_sightline_photons; mcrat_amd/csrc/sightline.hip) against tests/sightline_checker.py, an independent NumPy restatement of the
definitions (include/mcrat_hip.h) that finds the cell by brute force and takes kappa in the reference's form.

Exact: steps, status, surface_step, n_status, and -- bit for bit -- path and the surface point, for every ray the checker can judge.  A ray is
fragile when the checker says that a decision hangs on the last bits (a midpoint within 1e-9 of a cell's size of a face, a tau within the error bound
of tau_stop or of the surface level); for those only "status is a legal value" is asserted, and tests/test_sightline_checker_cpu.py holds the
condition that no case has more than one.

tau:  |tau_dev - tau_chk| <= sum_k 2 bar_k t_k + (K + 2) 2^-53 sum_k t_k,  t_k = kappa_k h_k of the checker.  bar_k is the conditioning bar that
tests/test_gpu_loop_arithmetic.py (_tau_bar_and_exact) derives for optical_depth_staged, restated in the checker:
    bar = (8u (1 + |x|)(1 + Gamma^2) + 2u |cos| / (Gamma^2 beta_g)) / (1 - x),   x = beta_g cos(theta),   u = 2^-53
-- the roundoff of the operands of 1 - x (beta_g / |v|: 4u (1 + Gamma^2); v.p: 2.5u; 1/|p|: 2 spacings) amplified by |x| / (1 - x), the subtraction's
own rounding and the products, and what the reference's beta_g costs near Gamma = 1; taken twice because both sides round.  The second term is
the worst case of adding K terms in any order plus the roundings of kappa_k h_k.  Derived, not measured; the largest error / bound is printed.
TABLE: sigma_hat = 10^z(log10 eps) multiplies kappa, and the comoving energy eps = Gamma_v (p0 - v.p) / (m_e c) carries the same cancellation as
1 - x: its relative error is within  bar_e = 8u (1 + |x_v|)(1 + Gamma_v^2) / (1 - x_v),  x_v = v.p / p0.  The test's table is linear in log10 eps with
slope b, so a relative error d of eps becomes (1 + d)^b - 1 ~ |b| d of sigma_hat: bar_k is widened by |b| bar_e -- the table's slope in log10 eps --
plus 16u (1 + |z|) ln 10 for the interpolation and the log10 / pow calls; in the cold branch sigma_hat = 1 - 2 eps moves by 2 eps bar_e."""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

EXACT_INT = ("steps", "status", "surface_step")


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


def engine_for(hip, c, frame=None):
    frame = c["frame"] if frame is None else frame
    e = hip.Engine(frame["dimensions"], frame["geometry"], 0, tau_calculation=hip.TAU_TABLE if c["table"] else hip.TAU_DIRECT)
    e.set_hydro(frame)
    if c["table"]:
        e.set_hot_cross_section(c["table"]["values"], c["table"]["grid"])
    return e


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same(a, b):
    """every output of two device runs, bit for bit"""
    for k in ("tau", "path", "surface_r"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    for k in EXACT_INT + ("n_status",):
        assert np.array_equal(a[k], b[k]), k


def compare(res, want, label):
    ok = ~want["fragile"]
    n_fragile = int(want["fragile"].sum())
    assert n_fragile <= 1, label
    for k in EXACT_INT:
        assert np.array_equal(res[k][ok], want[k][ok]), (label, k, np.nonzero(res[k] != want[k])[0][:8])
    assert np.array_equal(bits(res["path"][ok]), bits(want["path"][ok])), (label, "path")
    assert np.array_equal(bits(res["surface_r"][:, ok]), bits(want["surface_r"][:, ok])), (label, "surface_r")
    assert ((res["status"] >= 1) & (res["status"] <= 4)).all(), label
    assert np.array_equal(res["n_status"], np.bincount(res["status"], minlength=5)), label
    if n_fragile == 0:
        assert np.array_equal(res["n_status"], want["n_status"]), label
    err = np.abs(res["tau"] - want["tau"])[ok]
    bound = want["bound"][ok]
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
    print("%s: %d rays, %d fragile, largest tau error / bound = %.3g, largest relative tau error %.3g" %
          (label, len(ok), n_fragile, worst, float(np.max(err / np.maximum(want["tau"][ok], 1e-300), initial=0.0))))
    assert (err <= bound).all(), (label, worst)              # (a ray without a counted step: bound 0, the device's tau must be 0)


def run_case(hip, name, **kw):
    c = sc.case(name)
    e = engine_for(hip, c)
    res = e.sightline_rays(c["r"], c["p"], **c["params"], **kw)
    e.close()
    return c, res


# ---------------------------------------------------------------------------------------------- caller rays
@pytest.mark.parametrize("n", [1, 63, 65, 1000])
def test_ragged_sizes_uniform_steps(hip, monkeypatch, n):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c, res = run_case(hip, "uniform_n%d" % n)
    assert res["tau"].shape == (n,) and res["surface_r"].shape == (3, n) and res["n_status"].shape == (5,)
    compare(res, c["want"], "uniform steps, n = %d" % n)


@pytest.mark.parametrize("dims, geom", sc.PAIRS)
def test_every_dimensions_geometry_pair(hip, monkeypatch, dims, geom):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c, res = run_case(hip, "pair_%d_%d" % (dims, geom))
    compare(res, c["want"], "DIMENSIONS %d, geometry %d" % (dims, geom))
    assert c["want"]["steps"].max() > 60


@pytest.mark.parametrize("name", ["gap", "opaque", "cap_1", "cap_7", "surface_off", "gamma_100"])
def test_stops_and_surfaces(hip, monkeypatch, name):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c, res = run_case(hip, name)
    want = c["want"]
    compare(res, want, name)
    outside = (want["steps"] == 0) & (want["status"] == sc.LEFT_MESH)         # rays that start outside the domain
    assert outside.sum() >= 3 and (res["steps"][outside] == 0).all() and (res["tau"][outside] == 0).all() and (res["path"][outside] == 0).all()
    assert (res["status"][outside] == hip.SIGHTLINE_LEFT_MESH).all()
    if c["params"].get("surface_level", -1.0) >= 0:
        assert (res["surface_step"][outside] == 0).all() and np.array_equal(bits(res["surface_r"][:, outside]), bits(c["r"][:, outside]))
        other = res["status"] != hip.SIGHTLINE_LEFT_MESH
        assert (res["surface_step"][other] == -1).all() and np.isnan(res["surface_r"][:, other]).all()
    else:
        assert (res["surface_step"] == -1).all() and np.isnan(res["surface_r"]).all()
    if name == "opaque":
        assert (res["status"] == hip.SIGHTLINE_OPAQUE).sum() > 100 and (res["tau"][res["status"] == hip.SIGHTLINE_OPAQUE] >= 2.0).all()
    if name.startswith("cap"):
        assert (res["status"] == hip.SIGHTLINE_STEP_CAP).sum() > 200 and res["steps"].max() == c["params"]["max_steps"]


@pytest.mark.parametrize("name", ["uniform_n1000", "opaque", "pair_2_1"])
def test_refill_form_gives_the_same_bits(hip, monkeypatch, name):
    c = sc.case(name)
    e = engine_for(hip, c)
    monkeypatch.setenv("MCRAT_HIP_SIGHTLINE_REFILL", "0")
    plain = e.sightline_rays(c["r"], c["p"], **c["params"])
    monkeypatch.setenv("MCRAT_HIP_SIGHTLINE_REFILL", "1")
    refill = e.sightline_rays(c["r"], c["p"], **c["params"])
    same(plain, refill)
    compare(refill, c["want"], name + ", refill")
    monkeypatch.setenv("MCRAT_HIP_SIGHTLINE_REFILL", "yes")
    with pytest.raises(hip.McratHipError, match="MCRAT_HIP_SIGHTLINE_REFILL must be 0 or 1"):
        e.sightline_rays(c["r"], c["p"], **c["params"])
    e.close()


def test_refusals_reach_the_caller(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c = sc.case("uniform_n63")
    e = engine_for(hip, c)
    r, p = c["r"], c["p"]
    good = dict(step_frac=0.01, h_min=1e8, max_steps=16)
    for change, text in ((dict(step_frac=-1.0), "step_frac must be finite and not negative"), (dict(step_frac=np.nan), "step_frac must be finite"),
                         (dict(h_min=0.0), "h_min must be finite and positive"), (dict(h_min=np.inf), "h_min must be finite and positive"),
                         (dict(max_steps=0), "max_steps must lie between 1 and 1048576"), (dict(max_steps=(1 << 20) + 1), "max_steps must lie between"),
                         (dict(tau_stop=0.0), "tau_stop must be positive"), (dict(tau_stop=np.nan), "tau_stop must be positive"),
                         (dict(surface_level=np.inf), "surface_level must be a number below"), (dict(surface_level=np.nan), "surface_level must be a number below"),
                         (dict(step_frac=np.inf, h_min=-1.0, max_steps=0), "step_frac must be finite"),            # the first in order decides
                         (dict(max_steps=0, tau_stop=-1.0), "max_steps must lie between")):
        with pytest.raises(hip.McratHipError, match=text):
            e.sightline_rays(r, p, **dict(good, **change))
    with pytest.raises(hip.McratHipError, match="n must be at least 1"):
        e.sightline_rays(r[:, :0], p[:, :0], **good)
    with pytest.raises(hip.McratHipError, match="call out of order"):
        e.sightline_photons(**good)                               # no photons
    # a frame on a context with other switches
    other = hip.Engine(synth.TWO, synth.CARTESIAN, 0)
    other.set_hydro(dict(c["frame"], geometry=synth.CARTESIAN))
    with pytest.raises(hip.McratHipError, match="other switches"):
        e.sightline_rays(r, p, hydro=other, **good)
    tab = hip.Engine(synth.TWO, synth.CYLINDRICAL, 0, tau_calculation=hip.TAU_TABLE)
    tab.set_hydro(c["frame"])
    with pytest.raises(hip.McratHipError, match="other switches"):
        e.sightline_rays(r, p, hydro=tab, **good)
    with pytest.raises(hip.McratHipError, match="needs mcrat_hip_set_hot_cross_section first"):
        tab.sightline_rays(r, p, **good)                          # TABLE without a table
    bare = hip.Engine(synth.TWO, synth.CYLINDRICAL, 0)
    with pytest.raises(hip.McratHipError, match="no staged hydro frame"):
        bare.sightline_rays(r, p, **good)
    with pytest.raises(hip.McratHipError, match="no staged hydro frame"):
        e.sightline_rays(r, p, hydro=bare, **good)
    assert e.sightline_rays(r, p, **good)["n_status"].sum() == 63     # ... and the context still works
    for x in (other, tab, bare, e):
        x.close()


# ---------------------------------------------------------------------------------------------- resident photons
def photon_list(r, p, seed):
    n = r.shape[1]
    g = np.random.default_rng(seed)
    ph = {"r0": r[0].copy(), "r1": r[1].copy(), "r2": r[2].copy(), "p0": p[0].copy(), "p1": p[1].copy(), "p2": p[2].copy(), "p3": p[3].copy(),
          "s0": np.ones(n), "s1": np.zeros(n), "s2": np.zeros(n), "s3": np.zeros(n), "weight": 10.0 ** g.uniform(48.0, 51.0, n),
          "num_scatt": np.zeros(n), "time_to_scatter": np.zeros(n), "total_optical_depth": np.ones(n),
          "type": np.full(n, b"i", dtype="S1"), "nearest_block_index": np.zeros(n, dtype=np.int32), "recalc_properties": np.ones(n, dtype=np.int32)}
    for k in ("comv_p0", "comv_p1", "comv_p2", "comv_p3"):
        ph[k] = ph[k[5:]].copy()
    kind = g.integers(0, 10, n)
    ph["weight"][kind == 0] = 0.0
    ph["type"][kind == 1] = b"p"
    ph["type"][kind == 2] = b"N"
    ph["type"][kind == 3] = b"c"                       # other types are marched
    return ph, kind <= 2


def check_skipped(res, skipped, hip):
    assert (res["status"][skipped] == hip.SIGHTLINE_SKIPPED).all() and (res["status"][~skipped] != hip.SIGHTLINE_SKIPPED).all()
    for k in ("tau", "path", "steps"):
        assert not res[k][skipped].any(), k
    assert (res["surface_step"][skipped] == -1).all() and np.isnan(res["surface_r"][:, skipped]).all()
    assert res["n_status"][0] == skipped.sum() and res["n_status"].sum() == len(skipped)


@pytest.mark.parametrize("refill", ["0", "1"])
def test_resident_photons(hip, monkeypatch, refill):
    monkeypatch.setenv("MCRAT_HIP_SIGHTLINE_REFILL", refill)
    c = sc.case("photons")
    ph, skipped = photon_list(c["r"], c["p"], 5)
    assert 100 < skipped.sum() < 350
    e = engine_for(hip, c)
    e.set_photons(ph)
    before = e.get_photons()
    res = e.sightline_photons(**c["params"])
    after = e.get_photons()
    for k in before:                                       # the photon columns, bit for bit
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    check_skipped(res, skipped, hip)
    rays = e.sightline_rays(c["r"], c["p"], **c["params"])
    live = ~skipped
    for k in ("tau", "path"):
        assert np.array_equal(bits(res[k][live]), bits(rays[k][live])), k
    assert np.array_equal(bits(res["surface_r"][:, live]), bits(rays["surface_r"][:, live]))
    for k in EXACT_INT:
        assert np.array_equal(res[k][live], rays[k][live]), k
    compare(rays, c["want"], "photons as rays, refill " + refill)
    if not c["want"]["fragile"].any():
        assert np.array_equal(res["n_status"], sc.march(c["frame"], c["r"], c["p"], skip=skipped, **c["params"])["n_status"])
    e.close()


def test_pool_of_three_ragged_lists(hip, monkeypatch):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c = sc.case("photons")
    lens, ranks = [137, 300, 3], [0, 1, 3]                 # rank 2 is never created
    pool = engine_for(hip, c)
    pool.pool_create(4, 320)
    lists, first = [], 0
    for r, m in zip(ranks, lens):
        ph, skipped = photon_list(c["r"][:, first:first + m], c["p"][:, first:first + m], 40 + r)
        pool.pool_rank(r, r).set_photons(ph)
        lists.append((ph, skipped))
        first += m
    res = pool.pool_sightline_photons(**c["params"])
    stride = len(res["tau"]) // 4
    assert len(res["tau"]) == 4 * stride and stride >= 320
    covered = np.zeros(4 * stride, dtype=bool)
    total = np.zeros(5, dtype=np.int64)
    for r, m, (ph, skipped) in zip(ranks, lens, lists):
        view = pool.pool_rank(r, r).sightline_photons(**c["params"])
        assert len(view["tau"]) == m
        check_skipped(view, skipped, hip)
        sl = slice(r * stride, r * stride + m)
        for k in ("tau", "path"):
            assert np.array_equal(bits(res[k][sl]), bits(view[k])), (r, k)
        assert np.array_equal(bits(res["surface_r"][:, sl]), bits(view["surface_r"])), r
        for k in EXACT_INT:
            assert np.array_equal(res[k][sl], view[k]), (r, k)
        covered[sl] = True
        total += view["n_status"]
    assert (res["status"][~covered] == hip.SIGHTLINE_SKIPPED).all() and not res["tau"][~covered].any() and not res["steps"][~covered].any()
    total[0] += (~covered).sum()
    assert np.array_equal(res["n_status"], total) and total[1:].sum() > 250
    with pytest.raises(hip.McratHipError):
        pool.sightline_photons(**c["params"])              # the pool itself is not one list
    pool.close()


def test_frame_of_another_context(hip, monkeypatch):
    """the photons' own context holds only their slab, which a ray leaves at once; a second context holds the whole frame"""
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c = sc.case("larger_frame")
    whole = c["frame"]
    slab = synth.select_slab(whole, whole["r1"] < 1.04e12)
    ph, skipped = photon_list(c["r"], c["p"], 9)
    own = engine_for(hip, c, slab)
    own.set_photons(ph)
    big = engine_for(hip, c)
    through_slab = own.sightline_photons(**c["params"])
    through_whole = own.sightline_photons(hydro=big, **c["params"])
    own.set_hydro(whole)                                   # ... against staging that frame on the context itself
    same(through_whole, own.sightline_photons(**c["params"]))
    check_skipped(through_whole, skipped, hip)
    rays = own.sightline_rays(c["r"], c["p"], hydro=big, **c["params"])
    compare(rays, c["want"], "another context's frame")
    live = ~skipped
    assert np.array_equal(bits(rays["tau"][live]), bits(through_whole["tau"][live]))
    assert (through_slab["steps"] <= through_whole["steps"]).all() and (through_slab["steps"][live] < through_whole["steps"][live]).sum() > 100
    own.close()
    big.close()


# ---------------------------------------------------------------------------------------------- TAU_CALCULATION == TABLE
@pytest.mark.parametrize("name", ["table_in", "table_off", "table_cold"])
def test_table(hip, monkeypatch, name):
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)
    c, res = run_case(hip, name)
    want = c["want"]
    compare(res, want, name)
    off = res["status"] == hip.SIGHTLINE_OFF_TABLE
    if name == "table_off":
        assert off.sum() > 50 and (res["steps"][off] > 0).sum() > 30 and (res["tau"][off & (res["steps"] > 0)] > 0).all()
        assert res["n_status"][4] == off.sum()
    else:
        assert not off.any()
    # the table matters: the same rays in a DIRECT context give another tau
    direct = sc.march(c["frame"], c["r"], c["p"], **c["params"])
    marched = want["steps"] > 0
    assert (np.abs(direct["tau"] - want["tau"])[marched] > 100 * want["bound"][marched]).sum() > 100
