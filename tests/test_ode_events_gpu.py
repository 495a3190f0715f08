"""MassActionODELogLike(events=...) on the MI355X: the kernels with dosing and wash-out events give the host build's bits -- one lane
per item with neighbouring lanes holding different event counts (also where some conditions of a point fail), a lane group per item with
the groups of a wave in different conditions, the single-experiment kernels of both shapes --, run_dream equals the oracle driven by
the host build, and an object built with events=[] is the object built without the keyword."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_event_networks as EN
from . import ode_networks as NW
from . import ode_wide_networks as W
from .ode_support import device_equals_host, device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("max_steps", [500, EN.MM_STARVED_MAX_STEPS])
def test_one_lane_items_with_different_event_counts_equal_the_host_build(max_steps):
    """MM under 3 conditions with 0, 1 and 3 events: 131 points x 3 = 393 items, one full block and a partial one; neighbouring lanes hold
    different event counts.  At the small step limit there are points that fail in every condition, in some, in none."""
    multi, _ = EN.mm_conditions(max_steps=max_steps)
    X = NW.box_points(NW.MM_NOMINAL, 131, 21, width=1.0, outside=0.05)
    host = device_equals_host(multi, X, NW.MM_NOMINAL)
    count = np.sum(multi.batch_conditions(X) == -np.inf, axis=1)
    print("MM x 3 with 0, 1, 3 events at max_steps %d: points failing in all / some / no conditions: %d / %d / %d"
          % (max_steps, np.sum(count == 3), np.sum((count > 0) & (count < 3)), np.sum(count == 0)))
    if max_steps == 500:
        assert np.all(np.isfinite(host))
    else:
        assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)


def test_group_items_with_different_event_counts_equal_the_host_twin():
    """enzyme13 at 16 lanes x 3 conditions with 0, 1 and 3 events: 67 points = 201 items, 16 to a block -- the last block has groups
    without an item, and the four groups of a wave hold different conditions."""
    multi, _ = EN.enzyme13_conditions()
    assert multi.lanes_per_point == 16 and "EVENTS = 3" in multi.source()
    host = device_equals_host(multi, NW.box_points(W.ENZ.NOMINAL, 67, 21, width=1.0), W.ENZ.NOMINAL)
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name,n", [("chain17", 37), ("mm", 259)])
def test_a_single_experiment_with_events_equals_the_host_build(name, n):
    """chain17 at 32 lanes with a wash-out and a set-to-value: 37 points, 8 to a block; MM through the one-lane single-experiment kernel:
    259 points, a full block and three lanes of a second."""
    like = EN.single(name)
    nominal = EN._network(name)[5]
    assert like.lanes_per_point == (32 if name == "chain17" else 1) and like.conditions is None and "EVENTS" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, n, 22, width=1.0, outside=0.05), nominal)
    assert np.all(np.isfinite(host))


def test_run_dream_with_events_on_the_device_equals_the_oracle(tmp_path):
    """MM under three conditions with 0, 1 and 3 events against run_dream's own sequence on the oracle with the host build as the Python
    likelihood."""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = EN.mm_conditions()
    nom = NW.MM_NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(78)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("mm_seed.npy", Z0)
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False, history_file="mm_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 56, N, G, **kw)


def test_an_object_built_with_no_events_runs_the_kernel_it_always_ran():
    X = NW.box_points(NW.MM_NOMINAL, 259, 23, width=1.0)
    plain, empty = NW.michaelis_menten(), NW.michaelis_menten(events=[])
    assert empty.code_object() == plain.code_object()              # (the same unit: one entry of the kernel cache)
    a, b = device_logp(plain, X, NW.MM_NOMINAL - 1.0, 2.0)[1], device_logp(empty, X, NW.MM_NOMINAL - 1.0, 2.0)[1]
    assert a.tobytes() == b.tobytes() == plain.batch(X).tobytes() and np.all(np.isfinite(a))
