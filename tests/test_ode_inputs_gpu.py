"""MassActionODELogLike(inputs=...) on the MI355X: the kernels with piecewise-linear input time courses give the host build's bits in the
four device shapes -- one lane per point and per item (neighbouring lanes holding different knot counts, also where some conditions of a
point fail), a lane group per item with the groups of a wave at different knot times, a group of 32 with the equilibration phase, a wave
per point with two inputs --, the prediction kernels give the host's trajectories, run_dream equals the oracle driven by the host build,
and an object built with inputs=[] is the object built without the keyword."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_input_networks as IN
from . import ode_networks as NW
from .ode_support import device_equals_host, device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


def test_one_lane_with_an_input_equals_the_host_build():
    """drive2, a single experiment: 259 points, a full block and three lanes of a second"""
    like, nominal = IN.single("drive2"), IN.network("drive2")["nominal"]
    assert like.lanes_per_point == 1 and like.conditions is None and "INPUTS = 1" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, 259, 22, width=1.0, outside=0.05), nominal)
    assert np.any(np.isfinite(host))


@pytest.mark.parametrize("max_steps", [500, IN.MM_STARVED_MAX_STEPS])
def test_one_lane_items_with_different_knot_counts_equal_the_host_build(max_steps):
    """MM + input under 3 conditions with tables of 2, 3 and 6 knots, the last also with 3 events: 131 points x 3 = 393 items;
    neighbouring lanes hold different knot counts.  At 500 every value is finite; at the starved limit there are points that fail in every
    condition, in some, in none."""
    multi, _ = IN.mm_conditions(max_steps=max_steps)
    nominal = IN.network("mm")["nominal"]
    X = NW.box_points(nominal, 131, 21, width=1.0)
    host = device_equals_host(multi, X, nominal)
    count = np.sum(multi.batch_conditions(X) == -np.inf, axis=1)
    print("MM + input x 3 at max_steps %d: points failing in all / some / no conditions: %d / %d / %d"
          % (max_steps, np.sum(count == 3), np.sum((count > 0) & (count < 3)), np.sum(count == 0)))
    if max_steps == 500:
        assert np.all(np.isfinite(host))
    else:
        assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)


def test_group_items_with_different_knot_times_equal_the_host_twin():
    """enzyme13 + input at 16 lanes x 3 conditions: 67 points = 201 items, 16 to a block -- the last block has idle groups, and the four
    groups of a wave hold different conditions and so different knot times"""
    multi, _ = IN.enzyme13_conditions()
    nominal = IN.network("enzyme13")["nominal"]
    assert multi.lanes_per_point == 16 and "INPUTS = 1" in multi.source()
    host = device_equals_host(multi, NW.box_points(nominal, 67, 21, width=1.0), nominal)
    assert np.all(np.isfinite(host))


def test_a_group_of_32_that_equilibrates_under_the_basal_input_equals_the_host_twin():
    """chain17 + input at 32 lanes, 37 points, 8 to a block, with equilibrate=True"""
    like, nominal = IN.single("chain17", equilibrate=True), IN.network("chain17")["nominal"]
    assert like.lanes_per_point == 32 and "EQUILIBRATE" in like.source() and "INPUTS = 1" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, 37, 22, width=1.0), nominal)
    assert np.any(np.isfinite(host))


def test_a_wave_per_point_with_two_inputs_equals_the_host_twin():
    """chain40 + 2 inputs at 64 lanes, 9 points: two full blocks of four waves and one with idle waves"""
    like, nominal = IN.single("chain40"), IN.network("chain40")["nominal"]
    assert like.lanes_per_point == 64 and "INPUTS = 2" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, 9, 23, width=1.0), nominal)
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name", ["drive2", "enzyme13 x 3"])
def test_the_prediction_kernels_give_the_host_builds_trajectories(name):
    if name == "drive2":
        like, nominal = IN.single("drive2"), IN.network("drive2")["nominal"]
    else:
        like, nominal = IN.enzyme13_conditions()[0], IN.network("enzyme13")["nominal"]
    X = NW.box_points(nominal, 21, 24, width=1.0)
    with like.device() as ev:
        sim, terms = ev.simulate(X, return_terms=True)
        assert sim.tobytes() == like.simulate(X).tobytes() and np.all(np.isfinite(sim))
        if like.conditions is not None:
            assert terms.tobytes() == ev.batch_conditions(X).tobytes() == like.batch_conditions(X).tobytes()
        else:
            assert terms.tobytes() == like.batch(X).tobytes()


def test_run_dream_with_inputs_on_the_device_equals_the_oracle(tmp_path):
    """MM + input under its three conditions against run_dream's own sequence on the oracle with the host build as the Python likelihood"""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = IN.mm_conditions()
    nom = IN.network("mm")["nominal"]
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(78)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("mm_seed.npy", Z0)
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False, history_file="mm_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 56, N, G, **kw)


def test_an_object_built_with_no_inputs_runs_the_kernel_it_always_ran():
    X = NW.box_points(NW.MM_NOMINAL, 259, 23, width=1.0)
    plain, empty = NW.michaelis_menten(), NW.michaelis_menten(inputs=[])
    assert empty.code_object() == plain.code_object()              # (the same unit: one entry of the kernel cache)
    a, b = device_logp(plain, X, NW.MM_NOMINAL - 1.0, 2.0)[1], device_logp(empty, X, NW.MM_NOMINAL - 1.0, 2.0)[1]
    assert a.tobytes() == b.tobytes() == plain.batch(X).tobytes() and np.all(np.isfinite(a))
