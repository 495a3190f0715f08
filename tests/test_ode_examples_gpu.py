"""The shipped washout and binding_cycle examples and the combination of events with Monomials (ode_monomial_networks' *_events specs) on
the MI355X: the kernels give the host build's bits in both shapes, run_dream with washout equals the oracle driven by the host build, and
washout on chain-group streams (multitry off: both streams carry generations; multitry 3: the redraw rounds) equals the oracle and the run
without them."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.examples.binding_cycle import binding_cycle_device as BC
from pydream_amd.examples.washout import washout_device as WO
from pydream_amd.parameters import SampledParam

from . import ode_monomial_networks as MN
from . import ode_networks as NW
from .ode_support import device_equals_host, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,n", [("washout", 131), ("binding_cycle", 67)])
def test_a_shipped_example_on_the_device_equals_the_host_build(name, n):
    """washout: 131 points x 4 items, one lane each, two full blocks and a partial one, every item with the wash-out's restart;
    binding_cycle: 67 points x 9 items, the constraint's term in item 0"""
    M = WO if name == "washout" else BC
    like = M.make_likelihood()
    assert like.lanes_per_point == 1 and len(like.conditions) == len(M.DOSES)
    host = device_equals_host(like, NW.box_points(M.NOMINAL, n, 24, width=1.0, outside=0.05), M.NOMINAL)
    assert np.isfinite(host).sum() > n // 2


@pytest.mark.parametrize("name,lanes,n", [("mm_kd_events", 1, 131), ("mm_kd_events", 16, 131), ("enzyme13_m_events", 16, 67), ("chain17_m_events", 32, 37)])
def test_events_with_monomials_on_the_device_equal_the_host_build(name, lanes, n):
    """an event at t0 on the species whose start is a Monomial, events on and between output times, padded event blocks: one lane per
    item with neighbouring lanes in different conditions, and lane groups whose last block has groups without an item"""
    like, _ = MN.build(name, lanes_per_point=lanes)
    nominal = MN.nominal(name)
    assert like.lanes_per_point == lanes and "EVENTS" in like.source() and "MONOMIALS" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, n, 25, width=1.0, outside=0.05), nominal)
    assert np.isfinite(host).sum() > n // 2


def test_run_dream_with_washout_on_the_device_equals_the_oracle(tmp_path):
    """run_dream's own sequence on the oracle with the host build as the Python likelihood: 8 chains, 40 generations, multitry 3, no
    hard boundaries (redraw rounds through the items kernel)"""
    os.chdir(tmp_path)
    N, G = 8, 40
    like = WO.make_likelihood()
    nom = WO.NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(79)
    np.save("washout_seed.npy", nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom))))
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(like.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, history_thin=1, hardboundaries=False, history_file="washout_seed.npy")
    run_dream_equals_oracle(like, params, starts, 57, N, G, **kw)


@pytest.mark.parametrize("multitry", [1, 3])
def test_washout_on_chain_group_streams_equals_the_oracle(multitry, monkeypatch):
    """tests/test_module_modes_gpu.py's streams test with a real items likelihood: 128 chains (64 x 2: the fewest that keep two streams),
    DZ_STREAMS=2, 12 generations, the host build as the oracle's callback; also equal to the run without DZ_STREAMS.
    An ODE likelihood is never always_finite, so with multitry 3 a whole proposal set can be impossible: redo_possible() holds and
    one_generation sends such generations down ONE stream (the redraw rounds use shared buffers) -- that run covers the redraw rounds
    through the items kernel with the doubled d_items array, not the second slice.  With multitry off (1) no set is drawn again:
    every generation runs its two chain groups on their own streams, the second group's four items per point in the slice sl = 1 of
    d_items, added by k_sum_items from there."""
    from oracle import oracle as O
    from pydream_amd import _capi as G
    N, n, d = 128, 12, 3
    like = WO.make_likelihood()
    rng = np.random.default_rng(80)
    Z0 = WO.NOMINAL - 1.0 + 2 * rng.uniform(0, 1, (2 * N + 40, d))
    out = []
    for Cls, streams in ((G.Engine, None), (G.Engine, "2"), (O.Engine, None)):
        if streams is None:
            monkeypatch.delenv("DZ_STREAMS", raising=False)
        else:
            monkeypatch.setenv("DZ_STREAMS", streams)
        e = Cls(nchains=N, ndim=d, multitry=multitry, history_capacity=len(Z0) + N * (n // 4 + 2), trace_capacity=n, seed=81, history_thin=4,
                adapt_crossover=1, crossover_burnin=6, hardboundaries=0)
        e.set_prior(np.full(d, 2, np.int32), WO.NOMINAL - 1.0, np.full(d, 2.0))
        e.set_history(Z0); e.set_state(Z0[:N])
        if Cls is G.Engine:
            like._dz_apply(e)
        else:
            e.set_likelihood_host(lambda X: (np.zeros(len(X)), like.batch(X)))
        e.step(n // 2); e.step(n - n // 2)
        out.append((e.get_trace(0, n), e.get_history(), e.get_cr_state(), e.redraw_rounds() if Cls is G.Engine else None))
        e.close()
    for other in (out[0], out[2]):
        for key in ("snooker", "cr_idx", "try_idx", "moved", "X", "logp"):
            np.testing.assert_array_equal(out[1][0][key], other[0][key], err_msg=key)
        np.testing.assert_array_equal(out[1][1], other[1])
        for u, v in zip(out[1][2], other[2]):
            np.testing.assert_array_equal(u, v)
    assert (out[1][3] > 0) == (multitry == 3) and 0.02 < out[1][0]["moved"].mean() < 0.95
    assert np.all(np.isfinite(out[1][0]["logp"]))
