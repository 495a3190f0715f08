"""The features of MassActionODELogLike TOGETHER on the MI355X: on the seeded networks of tests/ode_combined_networks.py -- conditions,
Monomials, events, equilibrate, RateLaw/Hill, Noise and Input in one object -- the likelihood kernels of the four device shapes give the
host build's bits (launches of a full block plus a ragged one, rows outside the prior's box, dead rows, a single point, starved step
limits that fail a mix of the items of a wave), the prediction kernels give the host's trajectories and terms and fill NaN exactly where
an item is -inf, and run_dream equals the oracle driven by the host build.  The host build itself is held to the references in
test_ode_combined_cpu.py."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_combined_networks as CB
from .ode_support import device_equals_host, device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu

ALL = list(range(len(CB.CASES)))
IDS = [CB.case(i).name for i in ALL]
FULL_IDS = [CB.case(i).name for i in CB.FULL]


@pytest.mark.parametrize("i", ALL, ids=IDS)
def test_the_kernels_of_the_combination_equal_the_host_build(i):
    """CB.GPU_POINTS points x 3 conditions (393 items at one lane: neighbouring lanes in different conditions; 201 groups of 16 and 111
    of 32: idle groups in the last block; 27 waves, 15 at S = 64: idle waves), a margin outside the prior's box; then a single point;
    then the point with the dead rows, each of which is -inf"""
    c = CB.case(i)
    like = c.like()
    X = CB.gpu_points(c.lanes, c)
    host = device_equals_host(like, X, c.nominal, width=0.5)
    assert np.isfinite(host).sum() >= len(X) // 2
    device_equals_host(like, X[:1], c.nominal, width=0.5)
    rows = np.vstack([X[:1]] + [x for _, x in c.dead_rows()])          # (the likelihood alone: what the prior says of a NaN is not the point)
    lk = device_logp(like, rows, c.nominal - 0.5, 1.0)[1]
    assert lk.tobytes() == like.batch(rows).tobytes() and np.all(lk[1:] == -np.inf)


@pytest.mark.parametrize("lanes", [1, 16, 32, 64])
def test_starved_limits_fail_a_mix_of_the_items_of_a_wave(lanes):
    """the small full case of the build at CB.STARVED: some points fail in every condition, some in a few, some in none, some in the
    phase of condition 0 and some in an experiment alone (asserted on the host values, as in test_ode_combined_cpu.py) -- failed and
    finished items share a wave (64 lanes: a block)"""
    c, X = CB.starved_case(lanes), CB.starved_points(lanes)
    max_steps, phase_steps = CB.STARVED[lanes]
    like = c.like(max_steps=max_steps, equilibrate=dict(max_steps=phase_steps))
    device_equals_host(like, X, c.nominal, width=1.0)
    count = np.sum(like.batch_conditions(X) == -np.inf, axis=1)
    assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)


@pytest.mark.parametrize("i", CB.FULL, ids=FULL_IDS)
def test_the_prediction_kernels_of_the_combination_give_the_host_builds_bytes(i):
    """simulate(X, return_terms=True) through like.device(): the trajectories of the host's simulate, the terms of batch_conditions, NaN
    exactly in the slices of the items that are -inf -- dead rows and, at the starved limits of the small cases, failed items"""
    c = CB.case(i)
    starved = c is CB.starved_case(c.lanes)
    like = c.like(**(dict(max_steps=CB.STARVED[c.lanes][0], equilibrate=dict(max_steps=CB.STARVED[c.lanes][1])) if starved else {}))
    X = np.vstack([CB.starved_points(c.lanes)[:21] if starved else CB.gpu_points(c.lanes, c)[:21]] + [x for _, x in c.dead_rows()])
    with like.device() as ev:
        sim, terms = ev.simulate(X, return_terms=True)
    assert sim.tobytes() == like.simulate(X).tobytes() and terms.tobytes() == like.batch_conditions(X).tobytes()
    failed = terms == -np.inf
    assert failed.any() and not failed.all() and np.all(failed[-len(c.dead_rows()):])
    assert np.all(np.isnan(sim[failed])) and np.all(np.isfinite(sim[~failed]))


@pytest.mark.parametrize("lanes", [1, 16])
def test_run_dream_with_the_combination_on_the_device_equals_the_oracle(lanes, tmp_path):
    """8 chains, 40 generations, multitry 3 on the small full case against run_dream's own sequence on the oracle with the host build as
    the Python likelihood"""
    os.chdir(tmp_path)
    N, G = 8, 40
    c = CB.starved_case(lanes)
    like, nom = c.like(), c.nominal
    params = [SampledParam(uniform, loc=nom - 0.5, scale=1.0)]
    rng = np.random.default_rng(80 + lanes)
    np.save("combined_seed.npy", nom - 0.5 + rng.uniform(0, 1, (60, len(nom))))
    box = nom - 0.5 + rng.uniform(0, 1, (100, len(nom)))
    starts = list(box[np.isfinite(like.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False, history_file="combined_seed.npy")
    run_dream_equals_oracle(like, params, starts, 57 + lanes, N, G, **kw)
