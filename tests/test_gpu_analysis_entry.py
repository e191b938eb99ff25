"""The entry points of the analysis products that exist for one list and for a rank pool -- observe, sky, escaping, sky_resampled, events,
sightline_photons, radiation_field, comoving_field -- characterized from outside, product by product: which contexts each form refuses and with
what text, and that a view's call and its pool's call give the same bytes.  What the products compute is the subject of their own tests; this one
pins the plumbing that the sixteen entry points share (mcrat_amd/csrc/analysis_plan.hpp): where the photons come from, whose clocks they carry and
which identities (rank, slot) they get.

One stand-alone context with 64 photons; one pool of 2 lists x 64 slots whose only view, list 1, holds the same 64 photons, so that the pool's call
reads them at slots 64 .. 127 with rank 1 from slot / stride and the view's call at slots 0 .. 63 with rank 1 from the view; one context with a
frame and no photons.  The frame is the sightline checker's 16 x 16 cylindrical mesh, one observer, one bin per axis."""
import numpy as np
import pytest

from tests import escape_checker as ec
from tests import sightline_checker as sc

pytestmark = pytest.mark.gpu

PRODUCTS = ["observe", "sky", "escaping", "sky_resampled", "events", "sightline_photons", "radiation_field", "comoving_field"]
N, RANKS, LIST = 64, 2, 1
CLOCK = ec.TIME_NOW
T_EDGES, E_EDGES, TAU_EDGES = [0.0, 20.0], [1e-10, 1e-5], [0.0, 30.0]            # the photons are detected between 1 and 7 s (tests/escape_checker.py)
R_EDGES, MU_EDGES = [1.0e12, 1.2e12], [0.98, float(np.nextafter(1.0, 2.0))]
COMV_E_EDGES, COMV_A_EDGES = [1e-14, 1e-2], [-1.0, float(np.nextafter(1.0, 2.0))]

# the text of a list call on a pool
ON_A_POOL = {
    "observe": "observe: a rank pool's lists have clocks of their own",
    "sky": "observe_sky: a rank pool's lists have clocks of their own",
    "escaping": "observe_escaping: a rank pool's lists have clocks of their own",
    "sky_resampled": "observe_sky_resampled: a rank pool's lists have clocks of their own",
    "events": "observe_events: a rank pool's lists have clocks of their own",
    "sightline_photons": "sightline: one list is a stand-alone context or a view of a pool",
    "radiation_field": "radiation_field: one list is a stand-alone context or a view of a pool",
    "comoving_field": "comoving_field: one list is a stand-alone context or a view of a pool",
}
# the text of a pool call on a context that is no pool
NO_POOL = {
    "observe": "pool_observe: the context is no rank pool",
    "sky": "pool_observe_sky: the context is no rank pool",
    "escaping": "pool_observe_escaping: the context is no rank pool",
    "sky_resampled": "pool_observe_sky_resampled: the context is no rank pool",
    "events": "pool_observe_events: the context is no rank pool",
    "sightline_photons": "pool_sightline_photons: the context is no rank pool",
    "radiation_field": "pool_radiation_field: the context is no rank pool",
    "comoving_field": "pool_comoving_field: the context is no rank pool",
}
# the text of a list call on a context without photons: the observers' and the sightlines' calls return ESTATE without one
NO_PHOTONS = {"radiation_field": "radiation_field: no photons", "comoving_field": "comoving_field: no photons"}


@pytest.fixture(scope="module")
def hip():
    from mcrat_amd import engine
    engine.load_library()
    return engine


@pytest.fixture(autouse=True)
def no_switch(monkeypatch):
    for k in ("OBSERVE", "SKY", "ESCAPE", "RESAMPLE", "RADFIELD", "COMOVING"):
        monkeypatch.delenv("MCRAT_HIP_%s_PATH" % k, raising=False)
    monkeypatch.delenv("MCRAT_HIP_SIGHTLINE_REFILL", raising=False)


@pytest.fixture(scope="module")
def world(hip):
    """dict(case, alone, pool, view, bare): the contexts above, made once"""
    c = sc.CASES["uniform_n65"]()                      # (the frame and the rays; the checker's march is not needed here)
    ph = ec.photons_of(c, 4242, 0, N)

    def engine():
        e = hip.Engine(c["frame"]["dimensions"], c["frame"]["geometry"], 1)
        e.set_hydro(c["frame"])
        return e
    alone, pool, bare = engine(), engine(), engine()
    alone.set_photons(ph)
    # a caller who takes it for a pool of one list: the clocks' count passes, the context does not.  (The attribute is what Engine.pool_create sets;
    # a stand-alone Engine has none, so were it renamed the pool calls below would raise AttributeError, not the McratHipError the test asks for.)
    alone.n_pool_ranks = 1
    pool.pool_create(RANKS, N)
    view = pool.pool_rank(LIST, LIST)
    view.set_photons(ph)
    assert pool.n % RANKS == 0 and pool.n >= RANKS * N and view.n == N
    yield dict(case=c, alone=alone, pool=pool, view=view, bare=bare)
    for e in (alone, pool, bare):
        e.close()


def call(hip, world, product, e, pool):
    """`product` of context e: its list form at CLOCK, or its pool form with every list at CLOCK"""
    c = world["case"]
    march = ec.march_params(c["params"])
    clock = np.full(RANKS if e is world["pool"] else 1, CLOCK) if pool else CLOCK
    n, cos_acc, ex, ey = hip.sky_observers(0.05, 0.3, 0.5)
    f = lambda name: getattr(e, ("pool_" if pool else "") + name)
    if product == "observe":
        return f("observe")(*hip.observer_angles(5.0, 60.0), T_EDGES, E_EDGES, clock)
    if product == "sky":
        return f("observe_sky")(n, cos_acc, T_EDGES, E_EDGES, clock)
    if product == "escaping":
        return f("observe_escaping")(n, cos_acc, T_EDGES, E_EDGES, TAU_EDGES, clock, **march)
    if product == "sky_resampled":
        return f("observe_sky_resampled")(n, cos_acc, T_EDGES, E_EDGES, clock, mode=hip.RESAMPLE_JACKKNIFE, n_rep=4, stokes_frame=hip.STOKES_SKY_PLANE,
                                          seed=11, ex=ex, ey=ey)
    if product == "events":
        return f("observe_events")(n, cos_acc, clock, order=hip.EVENTS_BY_TIME, stokes_frame=hip.STOKES_SKY_PLANE, ex=ex, ey=ey)
    if product == "sightline_photons":
        return f("sightline_photons")(surface_level=c["params"]["surface_level"], **march)
    if product == "radiation_field":
        return f("radiation_field")(hip.RADFIELD_SHELLS, R_EDGES, MU_EDGES)
    assert product == "comoving_field"
    return f("comoving_field")(hip.COMOVING_SHELLS, COMV_E_EDGES, COMV_A_EDGES, R_EDGES, MU_EDGES)


@pytest.mark.parametrize("product", PRODUCTS)
def test_a_list_call_on_a_pool_is_refused(hip, world, product):
    with pytest.raises(hip.McratHipError, match=ON_A_POOL[product]):
        call(hip, world, product, world["pool"], pool=False)


@pytest.mark.parametrize("product", PRODUCTS)
def test_a_pool_call_on_a_stand_alone_context_is_refused(hip, world, product):
    with pytest.raises(hip.McratHipError, match=NO_POOL[product]):
        call(hip, world, product, world["alone"], pool=True)


@pytest.mark.parametrize("product", PRODUCTS)
def test_a_list_call_without_photons_is_refused(hip, world, product):
    with pytest.raises(hip.McratHipError, match=NO_PHOTONS.get(product)):
        call(hip, world, product, world["bare"], pool=False)


@pytest.mark.parametrize("product", PRODUCTS)
def test_the_view_and_its_pool_give_the_same_bytes(hip, world, product):
    of_view = call(hip, world, product, world["view"], pool=False)
    of_pool = call(hip, world, product, world["pool"], pool=True)
    assert of_view.keys() == of_pool.keys()
    if product == "sightline_photons":
        # one entry per slot of the pool, the view's rays from its list's first slot on; every other slot is skipped and counted as skipped
        first, skipped = LIST * (world["pool"].n // RANKS), hip.SIGHTLINE_SKIPPED
        mine = np.zeros(world["pool"].n, dtype=bool)
        mine[first:first + N] = True
        assert (of_pool["status"][~mine] == skipped).all() and of_pool["n_status"][skipped] == of_view["n_status"][skipped] + (~mine).sum()
        of_pool = {k: (v[..., mine] if k != "n_status" else v) for k, v in of_pool.items()}
        for r in (of_view, of_pool):
            r["n_status"] = np.delete(r["n_status"], skipped)
    for k in of_view:
        a, b = np.ascontiguousarray(of_view[k]), np.ascontiguousarray(of_pool[k])
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k        # (bytes: a NaN equals itself)
    # ... and they are not the same for want of photons
    if product == "events":
        assert of_view["n_total"] > 8 and (of_view["rank"] == LIST).all() and len(set(of_view["slot"])) == of_view["n_total"] and of_view["slot"].max() < N
    elif product == "sightline_photons":
        assert (of_view["status"] != hip.SIGHTLINE_SKIPPED).sum() > 8
    else:
        assert of_view["count"].sum() > 8
        if product == "sky_resampled":
            assert (of_view["count"] > 0).sum() > 1                # more than one jackknife group is populated: the identities matter
