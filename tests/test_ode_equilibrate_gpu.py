"""MassActionODELogLike(equilibrate=...) on the MI355X: the kernels with the equilibration phase give the host build's bits -- one
lane per item with neighbouring lanes in and out of the phase (also where the phase or the experiment is starved), a lane group per item
with the groups of a wave in different conditions, the single-experiment kernels of both shapes, a wave of 64 lanes per point --,
run_dream equals the oracle driven by the host build, and an object built with equilibrate=None is the object built without the keyword."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_equilibrate_networks as EQ
from . import ode_event_networks as EV
from . import ode_networks as NW
from . import ode_wave_networks as WV
from . import ode_wide_networks as W
from .ode_support import device_equals_host, device_logp, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("starved", [False, True])
def test_one_lane_items_in_and_out_of_the_phase_equal_the_host_build(starved):
    """MM under 3 conditions (phase off / on / on with a bolus at t0): 131 points x 3 = 393 items, one full block and a partial one;
    of three neighbouring lanes one skips the phase.  Starved -- the phase at EQ.MM_STARVED_EQUILIBRATE_STEPS attempts, the experiment
    at ode_event_networks' limit -- there are points that fail in every condition, in some, in none."""
    kw = dict(equilibrate=dict(max_steps=EQ.MM_STARVED_EQUILIBRATE_STEPS), max_steps=EV.MM_STARVED_MAX_STEPS) if starved else {}
    multi, _ = EQ.conditions("mm", **kw)
    assert multi.lanes_per_point == 1 and "EQUILIBRATE = true" in multi.source()
    X = NW.box_points(NW.MM_NOMINAL, 131, 21, width=1.0, outside=0.05)
    host = device_equals_host(multi, X, NW.MM_NOMINAL)
    count = np.sum(multi.batch_conditions(X) == -np.inf, axis=1)
    print("MM x 3 (phase off, on, on + bolus)%s: points failing in all / some / no conditions: %d / %d / %d"
          % (" starved" if starved else "", np.sum(count == 3), np.sum((count > 0) & (count < 3)), np.sum(count == 0)))
    if starved:
        assert np.any(count == 3) and np.any((count > 0) & (count < 3)) and np.any(count == 0)
    else:
        assert np.all(np.isfinite(host))


def test_group_items_in_and_out_of_the_phase_equal_the_host_twin():
    """enzyme13 at 16 lanes x 3 conditions: 67 points = 201 items, 16 to a block -- the last block has groups without an item, and the
    four groups of a wave are in different conditions, one of them outside the phase."""
    multi, _ = EQ.conditions("enzyme13")
    assert multi.lanes_per_point == 16 and "EQUILIBRATE = true" in multi.source()
    host = device_equals_host(multi, NW.box_points(W.ENZ.NOMINAL, 67, 21, width=1.0), W.ENZ.NOMINAL)
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name,n", [("chain17", 37), ("mm", 259)])
def test_a_single_experiment_with_the_phase_equals_the_host_build(name, n):
    """chain17 at 32 lanes: 37 points, 8 to a block; MM through the one-lane single-experiment kernel: 259 points, a full block and
    three lanes of a second.  Both with a bolus at t0 on the resting state."""
    like = EQ.single(name, events=[EQ.BOLUS[name]])
    nominal = EQ.network(name)[5]
    assert like.lanes_per_point == (32 if name == "chain17" else 1) and like.conditions is None and "EQUILIBRATE = true" in like.source()
    host = device_equals_host(like, NW.box_points(nominal, n, 22, width=1.0, outside=0.05), nominal)
    assert np.all(np.isfinite(host))


def test_a_wave_per_point_with_the_phase_equals_the_host_twin():
    """the smallest chain of ode_wave_networks.CASES: 9 points, two full blocks of four waves and a block with one"""
    name = EQ.smallest_wave_chain()
    like = EQ.single(name)
    assert like.lanes_per_point == 64 and like.n_species == min(c[3][0] for c in WV.CASES.values()) and "EQUILIBRATE = true" in like.source()
    host = device_equals_host(like, NW.box_points(WV.CHAIN_NOMINAL, 9, 23, width=1.0), WV.CHAIN_NOMINAL)
    assert np.all(np.isfinite(host))


def test_run_dream_with_the_phase_on_the_device_equals_the_oracle(tmp_path):
    """MM under the three conditions against run_dream's own sequence on the oracle with the host build as the Python likelihood."""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = EQ.conditions("mm")
    nom = NW.MM_NOMINAL
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(79)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("mm_seed.npy", Z0)
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=3, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=False, history_file="mm_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 57, N, G, **kw)


def test_an_object_built_without_the_phase_runs_the_kernel_it_always_ran():
    X = NW.box_points(NW.MM_NOMINAL, 259, 23, width=1.0)
    plain, none, off = NW.michaelis_menten(), NW.michaelis_menten(equilibrate=None), NW.michaelis_menten(equilibrate=False)
    assert none.code_object() == off.code_object() == plain.code_object()              # (the same unit: one entry of the kernel cache)
    a, b = device_logp(plain, X, NW.MM_NOMINAL - 1.0, 2.0)[1], device_logp(none, X, NW.MM_NOMINAL - 1.0, 2.0)[1]
    assert a.tobytes() == b.tobytes() == plain.batch(X).tobytes() and np.all(np.isfinite(a))
