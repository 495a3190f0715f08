"""likelihoods.Monomial on the MI355X: rate constants, start amounts, scales and constraints as monomials give the host build's bits on
the device -- one lane and a lane group per item, the single-experiment kernel, and where some conditions of a point fail -- and
run_dream with such a likelihood equals the oracle driven by the host build."""
import os

import numpy as np
import pytest
from scipy.stats import uniform

from pydream_amd.parameters import SampledParam

from . import ode_monomial_networks as MN
from . import ode_networks as NW
from .ode_support import device_equals_host, run_dream_equals_oracle

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,max_steps", [("mm_kd", 500), ("mm_kd", 60), ("mm_kd_doses", 60)])
def test_device_equals_host_build_one_lane_per_item(name, max_steps):
    """1027 points x 3 conditions = 3081 items (12 blocks and 9 items of a 13th).  With max_steps 60 points fail in some conditions and
    in none; mm_kd's last condition has no enzyme, nothing happens there and it cannot run out of steps, so points that fail in ALL
    conditions exist only with the enzyme in all three (mm_kd_doses), where all three kinds are required."""
    multi, _ = MN.build(name, max_steps=max_steps)
    nom = MN.nominal(name)
    X = NW.box_points(nom, 1027, 21, width=1.0, outside=0.05)
    host = device_equals_host(multi, X, nom)
    count = (multi.batch_conditions(X) == -np.inf).sum(axis=1)
    print("%s at max_steps %d: points failing in all / some / no conditions: %d / %d / %d"
          % (name, max_steps, np.sum(count == 3), np.sum((count > 0) & (count < 3)), np.sum(count == 0)))
    if max_steps == 500:
        assert np.all(np.isfinite(host))
    else:
        assert np.any((count > 0) & (count < 3)) and np.any(count == 0)
        assert np.any(count == 3) if name == "mm_kd_doses" else not np.any(count == 3)


def test_device_equals_host_build_single_experiment_long_form():
    """dense8_m: 24 reactions (the reaction-by-reaction source), 515 points = 2 blocks and 3 points, the constraints in the one-experiment kernel"""
    like, _ = MN.build("dense8_m")
    nom = MN.nominal("dense8_m")
    host = device_equals_host(like, NW.box_points(nom, 515, 21, width=1.0), nom)
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("name,n", [("enzyme13_m", 259), ("chain17_m", 131)])
def test_device_equals_host_twin_a_lane_group_per_item(name, n):
    """enzyme13_m@16: 259 points x 3 = 777 items, 16 to a block: the last block has groups without an item; chain17_m@32: 131 x 2 = 262, 8 to a block."""
    multi, _ = MN.build(name)
    nom = MN.nominal(name)
    host = device_equals_host(multi, NW.box_points(nom, n, 21, width=1.0), nom)
    assert np.all(np.isfinite(host))


@pytest.mark.parametrize("multitry,hard,max_steps", [(False, True, 500), (3, False, 60)])
def test_run_dream_on_the_device_equals_the_oracle(tmp_path, multitry, hard, max_steps):
    """mm_kd against run_dream's own sequence on the oracle with the host build as the Python likelihood; with max_steps 60 much of the
    prior box fails in at least one condition, so whole proposal sets are impossible and drawn again."""
    os.chdir(tmp_path)
    N, G = 8, 40
    multi, _ = MN.build("mm_kd", max_steps=max_steps)
    nom = MN.nominal("mm_kd")
    params = [SampledParam(uniform, loc=nom - 1.0, scale=2)]
    rng = np.random.default_rng(78)
    Z0 = nom - 1.0 + 2 * rng.uniform(0, 1, (60, len(nom)))
    np.save("mm_kd_seed.npy", Z0)
    if max_steps < 500:
        assert np.mean(multi.batch(Z0) == -np.inf) > 0.2
    box = nom - 1.0 + 2 * rng.uniform(0, 1, (200, len(nom)))
    starts = list(box[np.isfinite(multi.batch(box))][:N])
    assert len(starts) == N
    kw = dict(multitry=multitry, gamma_levels=4, adapt_gamma=True, history_thin=1, hardboundaries=hard, history_file="mm_kd_seed.npy")
    run_dream_equals_oracle(multi, params, starts, 56, N, G, **kw)
