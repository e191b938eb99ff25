"""mcrat_hip_device_bytes counts the device block of the ninth analysis product, the spectral fit (include/mcrat_hip.h: "HBM held by the context"):
its first call allocates the block -- the uploaded part, e_edges, log_e, count and w, and the result part, five double and three int columns -- and
the figure grows by at least what fit_plan.hpp lays out for it; a call with an equal or smaller need finds the block and leaves the figure alone, a
larger one makes it grow by at least the difference; the block is counted on the pool, not on a view.  The bytes are worked out here from the
documented layout -- without the padding between its parts, so they are a lower bound -- not read back from the library.  (The pattern of
tests/test_gpu_events_device_bytes.py.)"""
import numpy as np
import pytest

from mcrat_amd import synth
from tests import fit_checker as F
from tests import test_fit_plan_cpu as P

pytestmark = pytest.mark.gpu

N_E = 8


def need(n_spec, n_e=N_E):
    """the uploaded part: edges, log_e, count, w; the result part: alpha, beta, e_peak, amplitude, chi2, n_used, dof, status"""
    return 8 * (n_e + 1) + 8 * n_e + 2 * 8 * n_spec * n_e + 5 * 8 * n_spec + 3 * 4 * n_spec


def call(e, n_spec):
    rng = np.random.default_rng(n_spec)
    edges, _, count, w = P.synthetic(rng, F.COMP, n_spec, N_E, total=500.0)
    res = e.fit_spectra(count, w, edges, model=F.COMP, grid=(2, 2, 1), n_rounds=1, shrink=0.5)
    assert res["chi2"].shape == (n_spec,) and (res["n_used"] > 0).all()
    return res


def test_device_bytes_counts_the_fit_block():
    from mcrat_amd import engine
    engine.load_library()
    e = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    assert need(3) == 72 + 64 + 384 + 120 + 36
    before = e.device_bytes()
    first = call(e, 3)
    after = e.device_bytes()
    print("fit_spectra: device_bytes %d -> %d, the block needs at least %d" % (before, after, need(3)))
    assert after - before >= need(3)
    again = call(e, 3)
    assert e.device_bytes() == after
    for k in first:
        assert first[k].tobytes() == again[k].tobytes(), k                 # the block is reused and the result is the same
    call(e, 2)                                                             # (a smaller need: the block stays)
    assert e.device_bytes() == after
    call(e, 3 + 4000)                                                      # a larger one: it grows by at least the difference
    assert e.device_bytes() - after >= need(4003) - need(3) - 4096         # (less the padding the small block held)
    e.close()


def test_the_block_is_counted_on_the_pool_not_on_a_view():
    from mcrat_amd import engine
    engine.load_library()
    pool = engine.Engine(synth.TWO, synth.CYLINDRICAL, 1)
    pool.pool_create(2, 256)
    view = pool.pool_rank(0, 0)
    pool_before, view_before = pool.device_bytes(), view.device_bytes()
    on_view = call(view, 5)
    assert view.device_bytes() == view_before
    assert pool.device_bytes() - pool_before >= need(5)
    grown = pool.device_bytes()
    on_pool = call(pool, 5)
    assert pool.device_bytes() == grown and view.device_bytes() == view_before
    for k in on_view:
        assert on_view[k].tobytes() == on_pool[k].tobytes(), k
    pool.close()
